// Mesh decimation to a target face count: greedy quadric-error edge collapse (Garland-Heckbert), made parallel by collapsing an
// independent set of edges per round.  Semantics in include/nerf_hip.h "edge-collapse decimation"; tests/_decimate_ref.py
// reproduces every output bit for bit.  No reference counterpart.  The state (positions, quadrics, colour sums, merge counts, two
// face lists that take turns) lives in the workspace from nerf_decimate_begin on; per round the caller sorts twice and reads once:
//   keys      per corner of a face its half-edge key (min, max, direction) and its incidence key (vertex, face, corner).
//   (caller)  one sort of both rows.
//   edges     the vertices' rows from the incidence keys; the runs of the half-edge keys, ranked (count -> scan -> write, scan.h),
//             with the ends of every run that is not two opposed half-edges frozen.
//   quadrics  (first round only) per vertex the quadrics of its faces, summed in ascending face index.
//   select    candidate and cost per edge (two ring walks: the hot kernel); per pass the 64-bit minimum of the keys per vertex, the
//             minimum over each vertex's edges, the edges that are both ends' minimum, their neighbourhoods blocked.
//   (caller)  one sort of the selected keys.
//   apply     the trim threshold, the collapses (one lane per selected edge, one writer per vertex), the faces re-indexed and
//             compacted into the other list, the round's totals.
// No float atomics; the only atomics are 64-bit integer minima, and plain stores of equal values.  Launch- and cache-bound.
#include "lattice.h"
#include "quadric.h"
#include "scan.h"

namespace nerf {
namespace {

constexpr int DEC_BLOCK = 256;
constexpr int DEC_Q = 10;                           // A (xx, xy, xz, yy, yz, zz), b (3), c
constexpr int DEC_MAX_PASSES = 16;
constexpr int DEC_CNT = 8;                          // F, E, selected, candidates, frozen, V', trim threshold, F of the next round

typedef unsigned long long u64;
constexpr u64 DEC_NO_KEY = (u64)INT64_MAX;          // above every key: a cost's float32 bits are at most +inf's 0x7F800000
constexpr u64 DEC_MULT = 0x9E3779B1ull;

struct DecBox {
  double c[3], hs;                                  // the centre and half the longest side
};

// the workspace, carved on the host from (V, F) alone; H = 3 F half-edges bound the edges
struct DecWs {
  int64_t nblk_v, nblk_f, nblk_h;
  int64_t* cnt;                                     // [8]
  int64_t* blk_v;                                   // [nblk_v]
  int64_t* blk_f;                                   // [nblk_f]
  int64_t* blk_h;                                   // [nblk_h]
  double* Q;                                        // [V][10]
  double* col;                                      // [V][3]
  u64* m1;                                          // [V]
  u64* m2;                                          // [V]
  u64* ekey;                                        // [H]
  float* pos;                                       // [V][3]
  int* faces[2];                                    // [F][3] each
  int* mcnt;                                        // [V]
  int* remap;                                       // [V]
  int* vstart;                                      // [V], vend [V] right behind it
  int* vend;
  int* frozen;                                      // [V]
  int* blocked;                                     // [V]
  int* selend;                                      // [V]
  int* used;                                        // [V]
  int* newid;                                       // [V]
  int* ea;                                          // [H]
  int* eb;                                          // [H]
  int* sel;                                         // [H]
  int* inc;                                         // [H] face << 2 | corner, by ascending (vertex, face, corner)
  int64_t bytes;
};

DecWs dec_ws(void* ws, int64_t V, int64_t F) {
  DecWs w;
  const int64_t H = 3 * F;
  w.nblk_v = mesh_blocks(V, DEC_BLOCK);
  w.nblk_f = mesh_blocks(F, DEC_BLOCK);
  w.nblk_h = mesh_blocks(H, DEC_BLOCK);
  WsCarver<8> c(ws);
  w.cnt = c.take<int64_t>(DEC_CNT);
  w.blk_v = c.take<int64_t>(w.nblk_v);
  w.blk_f = c.take<int64_t>(w.nblk_f);
  w.blk_h = c.take<int64_t>(w.nblk_h);
  w.Q = c.take<double>(V * DEC_Q);
  w.col = c.take<double>(V * 3);
  w.m1 = c.take<u64>(V);
  w.m2 = c.take<u64>(V);
  w.ekey = c.take<u64>(H);
  w.pos = c.take<float>(V * 3);
  w.faces[0] = c.take<int>(F * 3);
  w.faces[1] = c.take<int>(F * 3);
  w.mcnt = c.take<int>(V);
  w.remap = c.take<int>(V);
  w.vstart = c.take<int>(2 * V);
  w.vend = w.vstart + V;
  w.frozen = c.take<int>(V);
  w.blocked = c.take<int>(V);
  w.selend = c.take<int>(V);
  w.used = c.take<int>(V);
  w.newid = c.take<int>(V);
  w.ea = c.take<int>(H);
  w.eb = c.take<int>(H);
  w.sel = c.take<int>(H);
  w.inc = c.take<int>(H);
  w.bytes = c.bytes();
  return w;
}

// u_a = ((double)v_a - ctr_a) / hs of vertex v; true when all three are finite
__device__ __forceinline__ bool dec_u(const float* __restrict__ pos, int v, const DecBox& bx, double* u) {
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float f = pos[3 * v + a];
    u[a] = ((double)f - bx.c[a]) / bx.hs;
    ok = ok && isfinite(f);
  }
  return ok;
}

__device__ __forceinline__ void dec_cross(const double* p0, const double* p1, const double* p2, double* n) {
  double e1[3], e2[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) { e1[a] = p1[a] - p0[a]; e2[a] = p2[a] - p0[a]; }
  n[0] = e1[1] * e2[2] - e1[2] * e2[1];
  n[1] = e1[2] * e2[0] - e1[0] * e2[2];
  n[2] = e1[0] * e2[1] - e1[1] * e2[0];
}

// the corners of face f after the remap; false for a face that goes (an index outside [0, V), two equal corners)
__device__ __forceinline__ bool dec_face(const int* __restrict__ faces, int f, int V, const int* __restrict__ remap, int* g) {
  if (!mesh_corners(faces + 3 * f, V, g)) return false;
#pragma unroll
  for (int c = 0; c < 3; ++c) g[c] = remap[g[c]];
  return mesh_distinct(g);
}

// ---- the state of the vertices: 12 (+ 12) B read, 12 + 8 (+ 24) B written per vertex
__global__ void __launch_bounds__(DEC_BLOCK) dec_init_kernel(const float* __restrict__ verts, const float* __restrict__ colors, int V,
                                                            float* __restrict__ pos, double* __restrict__ col, int* __restrict__ mcnt,
                                                            int* __restrict__ remap) {
  const int v = blockIdx.x * DEC_BLOCK + threadIdx.x;
  if (v >= V) return;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    pos[3 * v + a] = verts[3 * v + a];
    if (colors) col[3 * v + a] = (double)colors[3 * v + a];
  }
  mcnt[v] = 1;
  remap[v] = v;
}

// ---- the face remap: count (survivors per workgroup) and write (ranked inside the workgroup, in input order).  n_dev: the face
// count in device memory, else n_host.
__global__ void __launch_bounds__(DEC_BLOCK) dec_faces_count_kernel(const int* __restrict__ faces, const int64_t* __restrict__ n_dev,
                                                                   int64_t n_host, int V, const int* __restrict__ remap,
                                                                   int64_t* __restrict__ blk) {
  const int64_t F = n_dev ? n_dev[0] : n_host;
  const int f = blockIdx.x * DEC_BLOCK + threadIdx.x;
  int g[3];
  const int64_t t = block_sum<DEC_BLOCK>(f < F && dec_face(faces, f, V, remap, g) ? 1 : 0);
  if (threadIdx.x == 0) blk[blockIdx.x] = t;
}
__global__ void __launch_bounds__(DEC_BLOCK) dec_faces_write_kernel(const int* __restrict__ faces, const int64_t* __restrict__ n_dev,
                                                                   int64_t n_host, int V, const int* __restrict__ remap,
                                                                   const int64_t* __restrict__ blk, int64_t cap, int* __restrict__ out) {
  const int64_t F = n_dev ? n_dev[0] : n_host;
  const int f = blockIdx.x * DEC_BLOCK + threadIdx.x;
  int g[3] = {0, 0, 0};
  const int k = f < F && dec_face(faces, f, V, remap, g) ? 1 : 0;
  const int64_t id = block_offset<DEC_BLOCK>(k, blk[blockIdx.x]);
  if (!k || id >= cap) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) out[3 * id + c] = g[c];
}

// ---- keys: per corner i = 3 f + c the half-edge (g_c, g_c+1) as (min << 25) | (max << 1) | (g_c > g_c+1) and the incidence
// (g_c << 27) | (f << 2) | c; INT64_MAX behind the 3 F corners in use.  12 B read, 16 B written.
__global__ void __launch_bounds__(DEC_BLOCK) dec_keys_kernel(const int* __restrict__ faces, const int64_t* __restrict__ cnt, int64_t cap,
                                                            int64_t* __restrict__ hkeys, int64_t* __restrict__ ikeys) {
  const int64_t i = (int64_t)blockIdx.x * DEC_BLOCK + threadIdx.x;
  if (i >= cap) return;
  int64_t hk = INT64_MAX, ik = INT64_MAX;
  if (i < 3 * cnt[0]) {
    const int f = (int)(i / 3), c = (int)(i - 3 * (int64_t)f);
    const int64_t a = faces[3 * f + c], b = faces[3 * f + (c + 1) % 3];
    hk = ((a < b ? a : b) << 25) | ((a < b ? b : a) << 1) | (int64_t)(a > b);
    ik = (a << 27) | ((int64_t)f << 2) | (int64_t)c;
  }
  hkeys[i] = hk;
  ikeys[i] = ik;
}

// ---- rows: the first and one past the last sorted corner of every vertex (both arrays come in zeroed: a vertex without a
// face has an empty row); per sorted corner its face and corner.  8 B read, 4 B written per corner.
__global__ void __launch_bounds__(DEC_BLOCK) dec_rows_kernel(const int64_t* __restrict__ ikeys, const int64_t* __restrict__ cnt, int V,
                                                            int* __restrict__ inc, int* __restrict__ vstart, int* __restrict__ vend) {
  const int64_t H = 3 * cnt[0];
  const int64_t i = (int64_t)blockIdx.x * DEC_BLOCK + threadIdx.x;
  if (i >= H) return;
  const int64_t k = ikeys[i];
  const int64_t v = k >> 27;
  if (v < 0 || v >= V) return;                       // not this round's keys: write nothing through them
  inc[i] = (int)(k & ((1ll << 27) - 1));
  if (i == 0 || (ikeys[i - 1] >> 27) != v) vstart[v] = (int)i;
  if (i == H - 1 || (ikeys[i + 1] >> 27) != v) vend[v] = (int)i + 1;
}

// ---- edges: a run of half-edge keys with one (min, max) is one edge
__device__ __forceinline__ int dec_edge_head(const int64_t* __restrict__ hkeys, int64_t H, int64_t i) {
  return i < H && (i == 0 || (hkeys[i - 1] >> 1) != (hkeys[i] >> 1));
}
__global__ void __launch_bounds__(DEC_BLOCK) dec_edges_count_kernel(const int64_t* __restrict__ hkeys, const int64_t* __restrict__ cnt,
                                                                   int64_t* __restrict__ blk) {
  const int64_t t = block_sum<DEC_BLOCK>(dec_edge_head(hkeys, 3 * cnt[0], (int64_t)blockIdx.x * DEC_BLOCK + threadIdx.x));
  if (threadIdx.x == 0) blk[blockIdx.x] = t;
}
// per edge its ends at its rank; an end is frozen when the run is not exactly two half-edges of opposite direction, or when its
// own position is not finite (every writer stores the same value)
__global__ void __launch_bounds__(DEC_BLOCK) dec_edges_write_kernel(const int64_t* __restrict__ hkeys, const int64_t* __restrict__ cnt,
                                                                   const int64_t* __restrict__ blk, const float* __restrict__ pos,
                                                                   int V, int* __restrict__ ea, int* __restrict__ eb,
                                                                   int* __restrict__ frozen) {
  const int64_t H = 3 * cnt[0];
  const int64_t i = (int64_t)blockIdx.x * DEC_BLOCK + threadIdx.x;
  const int head = dec_edge_head(hkeys, H, i);
  const int64_t e = block_offset<DEC_BLOCK>(head, blk[blockIdx.x]);
  if (!head) return;
  const int64_t k = hkeys[i], pair = k >> 1;
  const int64_t a = pair >> 24, b = pair & ((1ll << 24) - 1);
  if (a < 0 || a >= V || b >= V) return;             // not this round's keys
  ea[e] = (int)a;
  eb[e] = (int)b;
  bool good = (k & 1) == 0 && i + 1 < H && hkeys[i + 1] == (k | 1);
  good = good && (i + 2 >= H || (hkeys[i + 2] >> 1) != pair);
  const bool fa = isfinite(pos[3 * a]) && isfinite(pos[3 * a + 1]) && isfinite(pos[3 * a + 2]);
  const bool fb = isfinite(pos[3 * b]) && isfinite(pos[3 * b + 1]) && isfinite(pos[3 * b + 2]);
  if (!good || !fa) frozen[a] = 1;
  if (!good || !fb) frozen[b] = 1;
}

// ---- initial quadrics: per vertex its row in ascending face index; a face adds when its three corners are finite.  Every face
// is evaluated once per corner, with the same bits.
__global__ void __launch_bounds__(DEC_BLOCK) dec_quadrics_kernel(const float* __restrict__ pos, const int* __restrict__ faces, int V,
                                                                const int* __restrict__ inc, const int* __restrict__ vstart,
                                                                const int* __restrict__ vend, DecBox bx, double* __restrict__ Q) {
  const int v = blockIdx.x * DEC_BLOCK + threadIdx.x;
  if (v >= V) return;
  double q[DEC_Q];
#pragma unroll
  for (int k = 0; k < DEC_Q; ++k) q[k] = 0.0;
  const int i1 = vend[v];
  for (int i = vstart[v]; i < i1; ++i) {
    const int f = inc[i] >> 2;
    double u0[3], u1[3], u2[3], n[3];
    const bool o0 = dec_u(pos, faces[3 * f], bx, u0), o1 = dec_u(pos, faces[3 * f + 1], bx, u1), o2 = dec_u(pos, faces[3 * f + 2], bx, u2);
    if (!o0 || !o1 || !o2) continue;
    dec_cross(u0, u1, u2, n);
    const double d = -((n[0] * u0[0] + n[1] * u0[1]) + n[2] * u0[2]);
    const double x[DEC_Q] = {n[0] * n[0], n[0] * n[1], n[0] * n[2], n[1] * n[1], n[1] * n[2], n[2] * n[2], n[0] * d, n[1] * d, n[2] * d, d * d};
#pragma unroll
    for (int k = 0; k < DEC_Q; ++k) q[k] = q[k] + x[k];
  }
#pragma unroll
  for (int k = 0; k < DEC_Q; ++k) Q[(int64_t)v * DEC_Q + k] = q[k];
}

// ---- placement and cost of the collapse of (a, b): q = Q[a] + Q[b] comes in; x and the cost go out
__device__ __forceinline__ double dec_place(const double* q, const double* ua, const double* ub, int quadric, double* x) {
  double m[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) x[a] = m[a] = (ua[a] + ub[a]) * 0.5;
  if (quadric) {
    const double d0 = ua[0] - ub[0], d1 = ua[1] - ub[1], d2 = ua[2] - ub[2];
    const double len2 = (d0 * d0 + d1 * d1) + d2 * d2;
    double s[3];                                     // accepted no farther from the midpoint than the edge is long
    if (quadric_solve(q, m, s)) {
      const double e0 = s[0] - m[0], e1 = s[1] - m[1], e2 = s[2] - m[2];
      const double dist2 = (e0 * e0 + e1 * e1) + e2 * e2;
      if (isfinite(s[0]) && isfinite(s[1]) && isfinite(s[2]) && dist2 <= len2) {
        x[0] = s[0]; x[1] = s[1]; x[2] = s[2];
      }
    }
  }
  const double ax0 = (q[0] * x[0] + q[1] * x[1]) + q[2] * x[2];
  const double ax1 = (q[1] * x[0] + q[3] * x[1]) + q[4] * x[2];
  const double ax2 = (q[2] * x[0] + q[4] * x[1]) + q[5] * x[2];
  const double xax = (x[0] * ax0 + x[1] * ax1) + x[2] * ax2;
  const double bx = (q[6] * x[0] + q[7] * x[1]) + q[8] * x[2];
  const double cost = (xax + 2.0 * bx) + q[9];
  return cost > 0.0 ? cost : 0.0;
}

// x and the cost of edge (a, b) from the state
__device__ __forceinline__ double dec_place_edge(const float* __restrict__ pos, const double* __restrict__ Q, int a, int b,
                                                 const DecBox& bx, int quadric, double* x) {
  double q[DEC_Q], ua[3], ub[3];
#pragma unroll
  for (int k = 0; k < DEC_Q; ++k) q[k] = Q[(int64_t)a * DEC_Q + k] + Q[(int64_t)b * DEC_Q + k];
  dec_u(pos, a, bx, ua);
  dec_u(pos, b, bx, ub);
  return dec_place(q, ua, ub, quadric, x);
}

// the faces of the row of v that do not hold `other`, with v moved to x: true when one of them loses its orientation
__device__ __forceinline__ bool dec_flips(const float* __restrict__ pos, const int* __restrict__ faces, const int* __restrict__ inc,
                                          int i0, int i1, int other, const DecBox& bx, const double* x) {
  bool bad = false;
  for (int i = i0; i < i1; ++i) {
    const int f = inc[i] >> 2, c = inc[i] & 3;
    const int g[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
    if (g[0] == other || g[1] == other || g[2] == other) continue;
    double p[3][3], q[3][3], n0[3], n1[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      dec_u(pos, g[j], bx, p[j]);
#pragma unroll
      for (int a = 0; a < 3; ++a) q[j][a] = j == c ? x[a] : p[j][a];
    }
    dec_cross(p[0], p[1], p[2], n0);
    dec_cross(q[0], q[1], q[2], n1);
    const double dot = (n0[0] * n1[0] + n0[1] * n1[1]) + n0[2] * n1[2];
    bad = bad || !(dot > 0.0);
  }
  return bad;
}

// ---- candidates: one lane per edge, two ring walks.  The key of a candidate, DEC_NO_KEY for every other edge.
__global__ void __launch_bounds__(DEC_BLOCK) dec_candidates_kernel(const float* __restrict__ pos, const double* __restrict__ Q,
                                                                  const int* __restrict__ faces, const int* __restrict__ inc,
                                                                  const int* __restrict__ vstart, const int* __restrict__ vend,
                                                                  const int* __restrict__ ea, const int* __restrict__ eb,
                                                                  const int* __restrict__ frozen, const int64_t* __restrict__ cnt,
                                                                  DecBox bx, int quadric, u64* __restrict__ ekey) {
  const int64_t e = (int64_t)blockIdx.x * DEC_BLOCK + threadIdx.x;
  if (e >= cnt[1]) return;
  const int a = ea[e], b = eb[e];
  u64 key = DEC_NO_KEY;
  if (!frozen[a] && !frozen[b]) {
    const int a0 = vstart[a], a1 = vend[a], b0 = vstart[b], b1 = vend[b];
    // the link condition: exactly two common neighbours, no ring edge opposite both ends
    int common = 0;
    bool clash = false;
    for (int i = a0; i < a1; ++i) {
      const int f = inc[i] >> 2, c = inc[i] & 3;
      const int na = faces[3 * f + (c + 1) % 3], pa = faces[3 * f + (c + 2) % 3];
      const bool sa = na == b || pa == b;
      const int la = min(na, pa), ha = max(na, pa);
      for (int j = b0; j < b1; ++j) {
        const int f2 = inc[j] >> 2, c2 = inc[j] & 3;
        const int nb = faces[3 * f2 + (c2 + 1) % 3], pb = faces[3 * f2 + (c2 + 2) % 3];
        common += na == nb;
        clash = clash || (!sa && nb != a && pb != a && la == min(nb, pb) && ha == max(nb, pb));
      }
    }
    if (common == 2 && !clash) {
      double x[3];
      const double cost = dec_place_edge(pos, Q, a, b, bx, quadric, x);
      if (!dec_flips(pos, faces, inc, a0, a1, b, bx, x) && !dec_flips(pos, faces, inc, b0, b1, a, bx, x))
        key = ((u64)__float_as_uint((float)cost) << 32) | (((u64)e * DEC_MULT) & 0xFFFFFFFFull);
    }
  }
  ekey[e] = key;
}

// ---- counts for the statistics: candidate keys over the E edges (the frozen and the used vertices: scan.h's flag count)
__global__ void __launch_bounds__(DEC_BLOCK) dec_count_keys_kernel(const u64* __restrict__ ekey, const int64_t* __restrict__ cnt,
                                                                  int64_t* __restrict__ blk) {
  const int64_t e = (int64_t)blockIdx.x * DEC_BLOCK + threadIdx.x;
  const int64_t t = block_sum<DEC_BLOCK>(e < cnt[1] && ekey[e] != DEC_NO_KEY ? 1 : 0);
  if (threadIdx.x == 0) blk[blockIdx.x] = t;
}

// ---- one selection pass.  An edge takes part when it is a candidate and neither end is blocked.
__device__ __forceinline__ bool dec_active(u64 key, int a, int b, const int* __restrict__ blocked) {
  return key != DEC_NO_KEY && !blocked[a] && !blocked[b];
}
// m1[v]: the minimum key over the edges at v that take part (m1 comes in as all ones)
__global__ void __launch_bounds__(DEC_BLOCK) dec_min1_kernel(const u64* __restrict__ ekey, const int* __restrict__ ea,
                                                            const int* __restrict__ eb, const int* __restrict__ blocked,
                                                            const int64_t* __restrict__ cnt, u64* m1) {
  const int64_t e = (int64_t)blockIdx.x * DEC_BLOCK + threadIdx.x;
  if (e >= cnt[1]) return;
  const int a = ea[e], b = eb[e];
  const u64 key = ekey[e];
  if (!dec_active(key, a, b, blocked)) return;
  atomicMin(&m1[a], key);
  atomicMin(&m1[b], key);
}
// m2[v] = min(m1[v], m1[u] over every edge (v, u)): every edge hands min(m1[a], m1[b]) to both ends (m2 comes in as all ones)
__global__ void __launch_bounds__(DEC_BLOCK) dec_min2_kernel(const int* __restrict__ ea, const int* __restrict__ eb,
                                                            const int64_t* __restrict__ cnt, const u64* __restrict__ m1, u64* m2) {
  const int64_t e = (int64_t)blockIdx.x * DEC_BLOCK + threadIdx.x;
  if (e >= cnt[1]) return;
  const int a = ea[e], b = eb[e];
  const u64 x = m1[a], y = m1[b];
  const u64 m = x < y ? x : y;
  if (m == ~0ull) return;
  atomicMin(&m2[a], m);
  atomicMin(&m2[b], m);
}
// selected iff the key is m2 of both ends; the ends are marked
__global__ void __launch_bounds__(DEC_BLOCK) dec_pick_kernel(const u64* __restrict__ ekey, const int* __restrict__ ea,
                                                            const int* __restrict__ eb, const int* __restrict__ blocked,
                                                            const int64_t* __restrict__ cnt, const u64* __restrict__ m2,
                                                            int* __restrict__ sel, int* __restrict__ selend) {
  const int64_t e = (int64_t)blockIdx.x * DEC_BLOCK + threadIdx.x;
  if (e >= cnt[1]) return;
  const int a = ea[e], b = eb[e];
  const u64 key = ekey[e];
  if (!dec_active(key, a, b, blocked) || key != m2[a] || key != m2[b]) return;
  sel[e] = 1;
  selend[a] = 1;
  selend[b] = 1;
}
// every vertex on an edge with an end of a selected edge is blocked, the ends included
__global__ void __launch_bounds__(DEC_BLOCK) dec_block_kernel(const int* __restrict__ ea, const int* __restrict__ eb,
                                                             const int64_t* __restrict__ cnt, const int* __restrict__ selend,
                                                             int* __restrict__ blocked) {
  const int64_t e = (int64_t)blockIdx.x * DEC_BLOCK + threadIdx.x;
  if (e >= cnt[1]) return;
  const int a = ea[e], b = eb[e];
  if (!selend[a] && !selend[b]) return;
  blocked[a] = 1;
  blocked[b] = 1;
}
// the selected keys for the caller's sort, DEC_NO_KEY elsewhere and behind the edges
__global__ void __launch_bounds__(DEC_BLOCK) dec_sel_keys_kernel(const u64* __restrict__ ekey, const int* __restrict__ sel,
                                                                const int64_t* __restrict__ cnt, int64_t cap, int64_t* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * DEC_BLOCK + threadIdx.x;
  if (e >= cap) return;
  out[e] = e < cnt[1] && sel[e] ? (int64_t)ekey[e] : (int64_t)DEC_NO_KEY;
}

// ---- trim: S = the selected keys (those below DEC_NO_KEY in the sorted list); if F - 2 S < target only the
// k = ceil((F - target) / 2) smallest stay.  cnt[2] = the collapses, cnt[6] = the largest key that stays.
__global__ void dec_trim_kernel(const int64_t* __restrict__ sorted, int64_t cap, int64_t target, int64_t* __restrict__ cnt) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int64_t lo = 0, hi = cap;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (sorted[mid] < (int64_t)DEC_NO_KEY) lo = mid + 1; else hi = mid;
  }
  int64_t S = lo, thr = (int64_t)DEC_NO_KEY - 1;
  const int64_t F = cnt[0];
  if (S > 0 && F - 2 * S < target) {
    int64_t k = (F - target + 1) / 2;
    k = k < 0 ? 0 : (k > S ? S : k);
    thr = k > 0 ? sorted[k - 1] : -1;
    S = k;
  }
  cnt[2] = S;
  cnt[6] = thr;
}

// ---- apply: one lane per selected edge.  No other collapse of the round reads or writes a or b (the header's proof).
__global__ void __launch_bounds__(DEC_BLOCK) dec_apply_kernel(const u64* __restrict__ ekey, const int* __restrict__ sel,
                                                             const int* __restrict__ ea, const int* __restrict__ eb,
                                                             const int64_t* __restrict__ cnt, DecBox bx, int quadric, float* pos,
                                                             double* Q, double* col, int* mcnt, int* __restrict__ remap) {
  const int64_t e = (int64_t)blockIdx.x * DEC_BLOCK + threadIdx.x;
  if (e >= cnt[1] || !sel[e] || (int64_t)ekey[e] > cnt[6]) return;
  const int a = ea[e], b = eb[e];
  double x[3];
  dec_place_edge(pos, Q, a, b, bx, quadric, x);
#pragma unroll
  for (int k = 0; k < 3; ++k) pos[3 * a + k] = (float)(bx.c[k] + x[k] * bx.hs);
#pragma unroll
  for (int k = 0; k < DEC_Q; ++k) Q[(int64_t)a * DEC_Q + k] = Q[(int64_t)a * DEC_Q + k] + Q[(int64_t)b * DEC_Q + k];
  if (col) {
#pragma unroll
    for (int k = 0; k < 3; ++k) col[3 * a + k] = col[3 * a + k] + col[3 * b + k];
  }
  mcnt[a] = mcnt[a] + mcnt[b];
  remap[b] = a;
}

// the round's totals (F', collapses, candidates, frozen vertices); F' becomes the face count
__global__ void dec_totals_kernel(int64_t* __restrict__ cnt, int64_t* __restrict__ totals) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  cnt[0] = cnt[7];
  totals[0] = cnt[7];
  totals[1] = cnt[2];
  totals[2] = cnt[3];
  totals[3] = cnt[4];
}

// ---- finish: the vertices the faces use, ranked in index order
__global__ void __launch_bounds__(DEC_BLOCK) dec_used_kernel(const int* __restrict__ faces, const int64_t* __restrict__ cnt,
                                                            int* __restrict__ used) {
  const int64_t i = (int64_t)blockIdx.x * DEC_BLOCK + threadIdx.x;
  if (i < 3 * cnt[0]) used[faces[i]] = 1;            // every writer stores the same value
}
__global__ void __launch_bounds__(DEC_BLOCK) dec_verts_write_kernel(const int* __restrict__ used, int V, const int64_t* __restrict__ blk,
                                                                   const float* __restrict__ pos, const double* __restrict__ col,
                                                                   const int* __restrict__ mcnt, int64_t V_out, int* __restrict__ newid,
                                                                   float* __restrict__ verts, float* __restrict__ colors) {
  const int v = blockIdx.x * DEC_BLOCK + threadIdx.x;
  const int u = v < V ? (used[v] != 0) : 0;
  const int64_t id = block_offset<DEC_BLOCK>(u, blk[blockIdx.x]);
  if (v >= V) return;
  newid[v] = u && id < V_out ? (int)id : -1;
  if (!u || id >= V_out) return;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    verts[3 * id + a] = pos[3 * v + a];
    if (colors) colors[3 * id + a] = (float)(col[3 * v + a] / (double)mcnt[v]);
  }
}
__global__ void __launch_bounds__(DEC_BLOCK) dec_faces_out_kernel(const int* __restrict__ faces, const int64_t* __restrict__ cnt,
                                                                 const int* __restrict__ newid, int64_t F_out, int* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * DEC_BLOCK + threadIdx.x;
  if (i < 3 * cnt[0] && i < 3 * F_out) out[i] = newid[faces[i]];
}

int dec_check(const char* who, int64_t V, int64_t F, int64_t F_cap, int parity) {
  NERF_REQUIRE(V >= 1 && V <= MESH_MAX_ITEMS && F >= 1 && F <= MESH_MAX_ITEMS, NERF_E_SHAPE,
               "%s: need 1 <= V, F <= 2^24 (got %lld, %lld)", who, (long long)V, (long long)F);
  NERF_REQUIRE(F_cap >= 1 && F_cap <= F, NERF_E_SHAPE, "%s: need 1 <= F_cap <= F (got %lld)", who, (long long)F_cap);
  NERF_REQUIRE(parity == 0 || parity == 1, NERF_E_SHAPE, "%s: the face list must be 0 or 1 (got %d)", who, parity);
  return NERF_OK;
}

int dec_box(const char* who, const float* lo, const float* hi, DecBox* bx) {
  const int rc = box_check(who, lo, hi);
  if (rc) return rc;
  double ext = 0.0;
  for (int a = 0; a < 3; ++a) {
    const double e = (double)hi[a] - (double)lo[a];
    ext = e > ext ? e : ext;
    bx->c[a] = ((double)lo[a] + (double)hi[a]) * 0.5;
  }
  bx->hs = ext * 0.5;
  return NERF_OK;
}

int dec_placement(const char* who, int placement) {
  NERF_REQUIRE(placement == NERF_DECIMATE_MIDPOINT || placement == NERF_DECIMATE_QUADRIC, NERF_E_SHAPE,
               "%s: placement must be 0 (midpoint) or 1 (quadric), got %d", who, placement);
  return NERF_OK;
}

#define DEC_LAUNCH(what, kernel, blocks, ...) NERF_LAUNCH(what, kernel, blocks, DEC_BLOCK, st, __VA_ARGS__)

}  // namespace
}  // namespace nerf

using namespace nerf;

extern "C" int64_t nerf_decimate_workspace_bytes(int64_t V, int64_t F) {
  if (V < 1 || V > MESH_MAX_ITEMS || F < 1 || F > MESH_MAX_ITEMS) return -1;
  return dec_ws(nullptr, V, F).bytes;
}

extern "C" int nerf_decimate_begin(const float* verts, const float* colors, int64_t V, const int32_t* faces, int64_t F, void* workspace,
                                   int64_t* totals, void* stream) {
  const char* who = "nerf_decimate_begin";
  NERF_TRY(dec_check(who, V, F, F, 0));
  NERF_REQUIRE(verts && faces && workspace && totals, NERF_E_NULL, "%s: NULL pointer", who);
  const DecWs w = dec_ws(workspace, V, F);
  hipStream_t st = as_stream(stream);
  DEC_LAUNCH("nerf_decimate_begin (vertices)", dec_init_kernel, w.nblk_v, verts, colors, (int)V, w.pos, colors ? w.col : (double*)nullptr,
             w.mcnt, w.remap);
  DEC_LAUNCH("nerf_decimate_begin (face counts)", dec_faces_count_kernel, w.nblk_f, faces, (const int64_t*)nullptr, F, (int)V,
             (const int*)w.remap, w.blk_f);
  NERF_TRY(scan_launch("nerf_decimate_begin (scan of the faces)", w.blk_f, w.nblk_f, w.cnt, st));
  DEC_LAUNCH("nerf_decimate_begin (faces)", dec_faces_write_kernel, w.nblk_f, faces, (const int64_t*)nullptr, F, (int)V,
             (const int*)w.remap, (const int64_t*)w.blk_f, F, w.faces[0]);
  NERF_HIP(who, hipMemcpyAsync(totals, w.cnt, sizeof(int64_t), hipMemcpyDeviceToDevice, st));
  return NERF_OK;
}

extern "C" int nerf_decimate_keys(int64_t V, int64_t F, int64_t F_cap, int parity, void* workspace, int64_t* keys, void* stream) {
  const char* who = "nerf_decimate_keys";
  NERF_TRY(dec_check(who, V, F, F_cap, parity));
  NERF_REQUIRE(workspace && keys, NERF_E_NULL, "%s: NULL pointer", who);
  const DecWs w = dec_ws(workspace, V, F);
  hipStream_t st = as_stream(stream);
  const int64_t cap = 3 * F_cap;
  DEC_LAUNCH(who, dec_keys_kernel, mesh_blocks(cap, DEC_BLOCK), (const int*)w.faces[parity], (const int64_t*)w.cnt, cap, keys, keys + cap);
  return NERF_OK;
}

extern "C" int nerf_decimate_edges(int64_t V, int64_t F, int64_t F_cap, const int64_t* sorted_keys, void* workspace, void* stream) {
  const char* who = "nerf_decimate_edges";
  NERF_TRY(dec_check(who, V, F, F_cap, 0));
  NERF_REQUIRE(workspace && sorted_keys, NERF_E_NULL, "%s: NULL pointer", who);
  const DecWs w = dec_ws(workspace, V, F);
  hipStream_t st = as_stream(stream);
  const int64_t cap = 3 * F_cap, nblk = mesh_blocks(cap, DEC_BLOCK);
  NERF_HIP(who, hipMemsetAsync(w.vstart, 0, 2 * V * sizeof(int), st));
  NERF_HIP(who, hipMemsetAsync(w.frozen, 0, V * sizeof(int), st));
  DEC_LAUNCH("nerf_decimate_edges (rows)", dec_rows_kernel, nblk, sorted_keys + cap, (const int64_t*)w.cnt, (int)V, w.inc, w.vstart, w.vend);
  DEC_LAUNCH("nerf_decimate_edges (run counts)", dec_edges_count_kernel, nblk, sorted_keys, (const int64_t*)w.cnt, w.blk_h);
  NERF_TRY(scan_launch("nerf_decimate_edges (scan of the runs)", w.blk_h, nblk, w.cnt + 1, st));
  DEC_LAUNCH("nerf_decimate_edges (runs)", dec_edges_write_kernel, nblk, sorted_keys, (const int64_t*)w.cnt, (const int64_t*)w.blk_h,
             (const float*)w.pos, (int)V, w.ea, w.eb, w.frozen);
  return NERF_OK;
}

extern "C" int nerf_decimate_quadrics(int64_t V, int64_t F, int parity, const float* lo, const float* hi, void* workspace, void* stream) {
  const char* who = "nerf_decimate_quadrics";
  DecBox bx;
  NERF_TRY(dec_check(who, V, F, F, parity));
  NERF_TRY(dec_box(who, lo, hi, &bx));
  NERF_REQUIRE(workspace, NERF_E_NULL, "%s: NULL pointer", who);
  const DecWs w = dec_ws(workspace, V, F);
  hipStream_t st = as_stream(stream);
  DEC_LAUNCH(who, dec_quadrics_kernel, w.nblk_v, (const float*)w.pos, (const int*)w.faces[parity], (int)V, (const int*)w.inc,
             (const int*)w.vstart, (const int*)w.vend, bx, w.Q);
  return NERF_OK;
}

extern "C" int nerf_decimate_select(int64_t V, int64_t F, int64_t F_cap, int parity, const float* lo, const float* hi, int placement,
                                    int passes, void* workspace, int64_t* sel_keys, void* stream) {
  const char* who = "nerf_decimate_select";
  DecBox bx;
  NERF_TRY(dec_check(who, V, F, F_cap, parity));
  NERF_TRY(dec_box(who, lo, hi, &bx));
  NERF_TRY(dec_placement(who, placement));
  NERF_REQUIRE(passes >= 1 && passes <= DEC_MAX_PASSES, NERF_E_SHAPE, "%s: need 1 <= passes <= %d (got %d)", who, DEC_MAX_PASSES, passes);
  NERF_REQUIRE(workspace && sel_keys, NERF_E_NULL, "%s: NULL pointer", who);
  const DecWs w = dec_ws(workspace, V, F);
  hipStream_t st = as_stream(stream);
  const int64_t cap = 3 * F_cap, nblk = mesh_blocks(cap, DEC_BLOCK);
  const int64_t* cnt = w.cnt;
  const int *ea = w.ea, *eb = w.eb;
  NERF_HIP(who, hipMemsetAsync(w.blocked, 0, V * sizeof(int), st));
  NERF_HIP(who, hipMemsetAsync(w.sel, 0, cap * sizeof(int), st));
  DEC_LAUNCH("nerf_decimate_select (candidates)", dec_candidates_kernel, nblk, (const float*)w.pos, (const double*)w.Q,
             (const int*)w.faces[parity], (const int*)w.inc, (const int*)w.vstart, (const int*)w.vend, ea, eb, (const int*)w.frozen, cnt,
             bx, placement, w.ekey);
  DEC_LAUNCH("nerf_decimate_select (candidate counts)", dec_count_keys_kernel, nblk, (const u64*)w.ekey, cnt, w.blk_h);
  NERF_TRY(scan_launch("nerf_decimate_select (scan of the candidates)", w.blk_h, nblk, w.cnt + 3, st));
  DEC_LAUNCH("nerf_decimate_select (frozen counts)", scan_flags_count_kernel<DEC_BLOCK>, w.nblk_v, (const int*)w.frozen,
             (const int64_t*)nullptr, V, w.blk_v);
  NERF_TRY(scan_launch("nerf_decimate_select (scan of the frozen)", w.blk_v, w.nblk_v, w.cnt + 4, st));
  for (int p = 0; p < passes; ++p) {
    NERF_HIP(who, hipMemsetAsync(w.m1, 0xFF, 2 * V * sizeof(u64), st));      // m1 and m2 are neighbours in the workspace
    NERF_HIP(who, hipMemsetAsync(w.selend, 0, V * sizeof(int), st));
    DEC_LAUNCH("nerf_decimate_select (vertex minima)", dec_min1_kernel, nblk, (const u64*)w.ekey, ea, eb, (const int*)w.blocked, cnt, w.m1);
    DEC_LAUNCH("nerf_decimate_select (ring minima)", dec_min2_kernel, nblk, ea, eb, cnt, (const u64*)w.m1, w.m2);
    DEC_LAUNCH("nerf_decimate_select (pick)", dec_pick_kernel, nblk, (const u64*)w.ekey, ea, eb, (const int*)w.blocked, cnt,
               (const u64*)w.m2, w.sel, w.selend);
    DEC_LAUNCH("nerf_decimate_select (block)", dec_block_kernel, nblk, ea, eb, cnt, (const int*)w.selend, w.blocked);
  }
  DEC_LAUNCH("nerf_decimate_select (selected keys)", dec_sel_keys_kernel, nblk, (const u64*)w.ekey, (const int*)w.sel, cnt, cap, sel_keys);
  return NERF_OK;
}

extern "C" int nerf_decimate_apply(int64_t V, int64_t F, int64_t F_cap, int parity, const float* lo, const float* hi, int placement,
                                   int has_colors, int64_t target, const int64_t* sorted_sel_keys, void* workspace, int64_t* totals,
                                   void* stream) {
  const char* who = "nerf_decimate_apply";
  DecBox bx;
  NERF_TRY(dec_check(who, V, F, F_cap, parity));
  NERF_TRY(dec_box(who, lo, hi, &bx));
  NERF_TRY(dec_placement(who, placement));
  NERF_REQUIRE(target >= 0, NERF_E_SHAPE, "%s: need target >= 0 (got %lld)", who, (long long)target);
  NERF_REQUIRE(workspace && sorted_sel_keys && totals, NERF_E_NULL, "%s: NULL pointer", who);
  const DecWs w = dec_ws(workspace, V, F);
  hipStream_t st = as_stream(stream);
  const int64_t cap = 3 * F_cap, nblk = mesh_blocks(cap, DEC_BLOCK), nblk_f = mesh_blocks(F_cap, DEC_BLOCK);
  const int64_t* cnt = w.cnt;
  hipLaunchKernelGGL(dec_trim_kernel, dim3(1), dim3(64), 0, st, sorted_sel_keys, cap, target, w.cnt);
  NERF_TRY(check_launch("nerf_decimate_apply (trim)"));
  DEC_LAUNCH("nerf_decimate_apply (collapses)", dec_apply_kernel, nblk, (const u64*)w.ekey, (const int*)w.sel, (const int*)w.ea,
             (const int*)w.eb, cnt, bx, placement, w.pos, w.Q, has_colors ? w.col : (double*)nullptr, w.mcnt, w.remap);
  DEC_LAUNCH("nerf_decimate_apply (face counts)", dec_faces_count_kernel, nblk_f, (const int*)w.faces[parity], cnt, (int64_t)0, (int)V,
             (const int*)w.remap, w.blk_f);
  NERF_TRY(scan_launch("nerf_decimate_apply (scan of the faces)", w.blk_f, nblk_f, w.cnt + 7, st));
  DEC_LAUNCH("nerf_decimate_apply (faces)", dec_faces_write_kernel, nblk_f, (const int*)w.faces[parity], cnt, (int64_t)0, (int)V,
             (const int*)w.remap, (const int64_t*)w.blk_f, F, w.faces[1 - parity]);
  hipLaunchKernelGGL(dec_totals_kernel, dim3(1), dim3(64), 0, st, w.cnt, totals);
  return check_launch("nerf_decimate_apply (totals)");
}

extern "C" int nerf_decimate_count(int64_t V, int64_t F, int64_t F_cap, int parity, void* workspace, int64_t* totals, void* stream) {
  const char* who = "nerf_decimate_count";
  NERF_TRY(dec_check(who, V, F, F_cap, parity));
  NERF_REQUIRE(workspace && totals, NERF_E_NULL, "%s: NULL pointer", who);
  const DecWs w = dec_ws(workspace, V, F);
  hipStream_t st = as_stream(stream);
  NERF_HIP(who, hipMemsetAsync(w.used, 0, V * sizeof(int), st));
  DEC_LAUNCH("nerf_decimate_count (used vertices)", dec_used_kernel, mesh_blocks(3 * F_cap, DEC_BLOCK), (const int*)w.faces[parity],
             (const int64_t*)w.cnt, w.used);
  DEC_LAUNCH("nerf_decimate_count (vertex counts)", scan_flags_count_kernel<DEC_BLOCK>, w.nblk_v, (const int*)w.used,
             (const int64_t*)nullptr, V, w.blk_v);
  NERF_TRY(scan_launch("nerf_decimate_count (scan of the vertices)", w.blk_v, w.nblk_v, w.cnt + 5, st));
  NERF_HIP(who, hipMemcpyAsync(totals, w.cnt + 5, sizeof(int64_t), hipMemcpyDeviceToDevice, st));
  NERF_HIP(who, hipMemcpyAsync(totals + 1, w.cnt, sizeof(int64_t), hipMemcpyDeviceToDevice, st));
  return NERF_OK;
}

extern "C" int nerf_decimate_write(int64_t V, int64_t F, int parity, int has_colors, void* workspace, int64_t V_out, int64_t F_out,
                                   float* verts_out, float* colors_out, int32_t* faces_out, void* stream) {
  const char* who = "nerf_decimate_write";
  NERF_TRY(dec_check(who, V, F, F, parity));
  NERF_REQUIRE(V_out >= 0 && V_out <= V && F_out >= 0 && F_out <= F, NERF_E_SHAPE, "%s: bad V_out %lld / F_out %lld", who,
               (long long)V_out, (long long)F_out);
  NERF_REQUIRE(!colors_out || has_colors, NERF_E_SHAPE, "%s: colours out of a state that was begun without colours", who);
  if (V_out == 0 && F_out == 0) return NERF_OK;
  NERF_REQUIRE(workspace && verts_out && faces_out, NERF_E_NULL, "%s: NULL pointer", who);
  const DecWs w = dec_ws(workspace, V, F);
  hipStream_t st = as_stream(stream);
  DEC_LAUNCH("nerf_decimate_write (vertices)", dec_verts_write_kernel, w.nblk_v, (const int*)w.used, (int)V, (const int64_t*)w.blk_v,
             (const float*)w.pos, (const double*)w.col, (const int*)w.mcnt, V_out, w.newid, verts_out, colors_out);
  if (F_out > 0)
    DEC_LAUNCH("nerf_decimate_write (faces)", dec_faces_out_kernel, mesh_blocks(3 * F_out, DEC_BLOCK), (const int*)w.faces[parity],
               (const int64_t*)w.cnt, (const int*)w.newid, F_out, faces_out);
  return NERF_OK;
}
