// Mesh simplification by vertex clustering with quadric placement (Rossignac-Borrel cells, Lindstrom's area^2-weighted quadrics):
// the decimation step behind marching cubes.  Semantics in include/nerf_hip.h "mesh simplification"; tests/_simplify_ref.py
// reproduces every output bit for bit.  No reference counterpart.  Three entries with the caller's stable sort and one host read
// between them:
//   cluster  keys and occupancy bit mask (one bit per cell, packed like morph.hip's masks) -> per-word prefix counts (count ->
//            block scan -> write, scan.h) -> ranks; the per-cluster sums as exact int64 atomics (any arrival order gives the same
//            bits); per face its quadric, its orientation and the 63-bit key of its sorted cluster triple.
//   count    on the sorted keys: run heads and the prefix of one orientation in one two-counter scan, survivors decided per
//            position from the run's two ends (linear in F whatever the run lengths), used clusters, both compactions' counts.
//   write    the placement solve of the used clusters and the renumbered surviving faces, ranked inside the workgroup.
// All HBM- or launch-bound.
#include "lattice.h"
#include "quadric.h"
#include "scan.h"

namespace nerf {
namespace {

constexpr int SIMP_BLOCK = 256;
constexpr int SIMP_ACC = 19;                        // n, S[3], N[3], C[3], Q[9]
constexpr int SIMP_KEY_BITS = 21;
constexpr int64_t SIMP_NO_KEY = INT64_MAX;          // a dropped face: sorts behind every triple (three equal ids are never a key)

typedef unsigned long long u64;

struct SBox {
  double lo[3], inv[3], c[3];
  int G;
};

// the workspace, carved on the host from (V, F, G) alone
struct SimpWs {
  int64_t W, nblk_w, K_max, nblk_c, nblk_f;
  u64* mask;                                        // [W] one bit per cell
  int64_t* acc;                                     // [K_max][19]
  int64_t* cnt;                                     // [4]: K, run heads, faces of the odd orientation, -
  int64_t* blk_w;                                   // [nblk_w]
  int64_t* blk_c;                                   // [nblk_c]
  int64_t* blk_s;                                   // [2][nblk_f] heads, odd faces
  int64_t* blk_f;                                   // [nblk_f]
  int* wpre;                                        // [W] clusters below the word
  int* vcid;                                        // [V] cluster of a vertex, -1 invalid
  int* ckey;                                        // [K_max] cell key of a cluster
  int* used;                                        // [K_max]
  int* newid;                                       // [K_max]
  int* odd;                                         // [F + 1] odd faces below a sorted position
  int* rid;                                         // [F] run of a sorted position
  int* heads;                                       // [F + 1] first position of a run
  int* keep;                                        // [F] by input order
  uint8_t* par;                                     // [F] orientation of a face, by input order
  int64_t bytes;
};

SimpWs simp_ws(void* ws, int64_t V, int64_t F, int G) {
  SimpWs w;
  const int64_t cells = (int64_t)G * G * G;
  w.W = (cells + 63) >> 6;
  w.nblk_w = mesh_blocks(w.W, SIMP_BLOCK);
  w.K_max = V < cells ? V : cells;
  w.nblk_c = mesh_blocks(w.K_max, SIMP_BLOCK);
  w.nblk_f = mesh_blocks(F, SIMP_BLOCK);
  WsCarver<8> c(ws);
  w.mask = c.take<u64>(w.W);
  w.acc = c.take<int64_t>(w.K_max * SIMP_ACC);
  w.cnt = c.take<int64_t>(4);
  w.blk_w = c.take<int64_t>(w.nblk_w);
  w.blk_c = c.take<int64_t>(w.nblk_c);
  w.blk_s = c.take<int64_t>(2 * w.nblk_f);
  w.blk_f = c.take<int64_t>(w.nblk_f);
  w.wpre = c.take<int>(w.W);
  w.vcid = c.take<int>(V);
  w.ckey = c.take<int>(w.K_max);
  w.used = c.take<int>(w.K_max);
  w.newid = c.take<int>(w.K_max);
  w.odd = c.take<int>(F + 1);
  w.rid = c.take<int>(F);
  w.heads = c.take<int>(F + 1);
  w.keep = c.take<int>(F);
  w.par = c.take<uint8_t>(F);
  w.bytes = c.bytes();
  return w;
}

// ---- the cell of a vertex.  t_a = (v_a - lo_a) inv_a; valid iff all three are finite; q_a = clamp(floor(t_a), 0, G - 1).
__device__ __forceinline__ bool cell_of(const float* __restrict__ verts, int v, const SBox& bx, double* t, double* q) {
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    t[a] = ((double)verts[3 * v + a] - bx.lo[a]) * bx.inv[a];
    ok = ok && isfinite(t[a]);
    q[a] = fmin(fmax(floor(t[a]), 0.0), (double)(bx.G - 1));
  }
  return ok;
}
__device__ __forceinline__ int key_of(const double* q, int G) { return ((int)q[2] * G + (int)q[1]) * G + (int)q[0]; }

__device__ __forceinline__ void add64(int64_t* p, int64_t v) {
  if (v) atomicAdd(reinterpret_cast<u64*>(p), (u64)v);
}

// v[c] summed over each run of consecutive lanes of the wave that hold the same key (key < 0: the lane has nothing to add); true
// in the last lane of a run with a key, whose v then holds the run's totals.  Marching cubes emits vertices and faces cell by cell,
// x fastest, so neighbouring lanes mostly share a cluster: one atomic per run instead of one per lane.  Integer sums: the grouping
// changes no bit.  With OR the values are combined with | instead of +.  EVERY lane of the wave must call it.
template <int N, bool OR = false>
__device__ __forceinline__ bool wave_run_sum(int key, int64_t (&v)[N]) {
  const int lane = threadIdx.x & 63;
  const int prev = __shfl_up(key, 1, WAVE);
  const u64 heads = __ballot(lane == 0 || prev != key);
  const int start = 63 - __clzll(heads & (~0ull >> (63 - lane)));      // the run's first lane
  for (int o = 1; o < WAVE; o <<= 1) {
    const bool take = lane - o >= start;
    if (!__any(take)) break;                          // wave-uniform: no run is longer than o lanes
#pragma unroll
    for (int c = 0; c < N; ++c) {
      const int64_t t = __shfl_up(v[c], o, WAVE);
      if (take) v[c] = OR ? (v[c] | t) : v[c] + t;
    }
  }
  return key >= 0 && (lane == 63 || ((heads >> (lane + 1)) & 1ull));
}

// ---- keys: 12 B read per vertex; one atomic OR per run of lanes on one mask word, unless its bits are seen set already (a stale
// read only costs the atomic).  vcid holds the key until the ranks.
__global__ void __launch_bounds__(SIMP_BLOCK) simp_keys_kernel(const float* __restrict__ verts, int V, SBox bx, u64* mask,
                                                              int* __restrict__ vcid) {
  const int v = blockIdx.x * SIMP_BLOCK + threadIdx.x;
  double t[3], q[3];
  int key = -1;
  if (v < V && cell_of(verts, v, bx, t, q)) key = key_of(q, bx.G);
  if (v < V) vcid[v] = key;
  const int word = key >> 6;                         // -1 without a key
  int64_t bits[1] = {key >= 0 ? (int64_t)(1ull << (key & 63)) : 0};
  if (!wave_run_sum<1, true>(word, bits)) return;
  const u64 b = (u64)bits[0];
  if ((mask[word] & b) != b) atomicOr(&mask[word], b);
}

// ---- per-word prefix counts: count (popcounts per workgroup of 256 words) and write (ranked inside the workgroup)
__global__ void __launch_bounds__(SIMP_BLOCK) simp_words_count_kernel(const u64* __restrict__ mask, int64_t W,
                                                                     int64_t* __restrict__ blk) {
  const int64_t w = (int64_t)blockIdx.x * SIMP_BLOCK + threadIdx.x;
  const int64_t t = block_sum<SIMP_BLOCK>(w < W ? __popcll(mask[w]) : 0);
  if (threadIdx.x == 0) blk[blockIdx.x] = t;
}
__global__ void __launch_bounds__(SIMP_BLOCK) simp_words_write_kernel(const u64* __restrict__ mask, int64_t W,
                                                                     const int64_t* __restrict__ blk, int* __restrict__ wpre) {
  const int64_t w = (int64_t)blockIdx.x * SIMP_BLOCK + threadIdx.x;
  const int64_t o = block_offset<SIMP_BLOCK>(w < W ? __popcll(mask[w]) : 0, blk[blockIdx.x]);
  if (w < W) wpre[w] = (int)o;
}

// ---- zero: the accumulators and the used flags of the K clusters (K from device memory: nothing is read on the host)
__global__ void __launch_bounds__(SIMP_BLOCK) simp_zero_kernel(const int64_t* __restrict__ cnt, int64_t* __restrict__ acc,
                                                              int* __restrict__ used) {
  const int64_t K = cnt[0];
  for (int64_t i = (int64_t)blockIdx.x * SIMP_BLOCK + threadIdx.x; i < K * SIMP_ACC; i += (int64_t)gridDim.x * SIMP_BLOCK) {
    acc[i] = 0;
    if (i < K) used[i] = 0;
  }
}

// ---- ranks and vertex sums: 12 + 12 (+ 12) B read per vertex; up to 10 integer atomics per run of lanes in one cluster
__global__ void __launch_bounds__(SIMP_BLOCK) simp_vertices_kernel(const float* __restrict__ verts, const float* __restrict__ normals,
                                                                  const float* __restrict__ colors, int V, SBox bx,
                                                                  const u64* __restrict__ mask, const int* __restrict__ wpre,
                                                                  int* __restrict__ vcid, int* __restrict__ ckey,
                                                                  int64_t* __restrict__ acc) {
  const int v = blockIdx.x * SIMP_BLOCK + threadIdx.x;
  const int key = v < V ? vcid[v] : -1;
  int cid = -1;
  int64_t s[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // n, S, N, C: the first ten sums of a cluster
  if (key >= 0) {
    cid = wpre[key >> 6] + __popcll(mask[key >> 6] & ((1ull << (key & 63)) - 1ull));
    vcid[v] = cid;
    ckey[cid] = key;                                 // every writer stores the same value
    double t[3], q[3];
    cell_of(verts, v, bx, t, q);
    s[0] = 1;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double u = t[a] - (q[a] + 0.5);
      s[1 + a] = fixed(u, 64.0, 4294967296.0);
      const float n = normals[3 * v + a];
      s[4 + a] = isfinite(n) ? fixed((double)n, 256.0, 1073741824.0) : 0;
      if (colors) {
        const float c = colors[3 * v + a];
        s[7 + a] = c != c ? 0 : (int64_t)rint(fmin(fmax((double)c, 0.0), 1.0) * 1073741824.0);
      }
    }
  }
  if (!wave_run_sum(cid, s)) return;
  int64_t* A = acc + (int64_t)cid * SIMP_ACC;
#pragma unroll
  for (int c = 0; c < 10; ++c) add64(A + c, s[c]);
}

// the nine quadric addends of the triangle (t0, t1, t2) in the local coordinates of cell q
__device__ __forceinline__ void quadric_of(const double (*t)[3], const double* q, int64_t (&x9)[9]) {
  double u[3][3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
#pragma unroll
    for (int a = 0; a < 3; ++a) u[j][a] = t[j][a] - (q[a] + 0.5);
  }
  double e1[3], e2[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) { e1[a] = u[1][a] - u[0][a]; e2[a] = u[2][a] - u[0][a]; }
  const double nx = e1[1] * e2[2] - e1[2] * e2[1];
  const double ny = e1[2] * e2[0] - e1[0] * e2[2];
  const double nz = e1[0] * e2[1] - e1[1] * e2[0];
  const double d = -((nx * u[0][0] + ny * u[0][1]) + nz * u[0][2]);
  const double x[9] = {nx * nx, nx * ny, nx * nz, ny * ny, ny * nz, nz * nz, nx * d, ny * d, nz * d};
#pragma unroll
  for (int k = 0; k < 9; ++k) x9[k] = fixed(x[k], 64.0, 4294967296.0);
}

// ---- faces: 12 B + three vertices read per face; its quadric once per distinct cluster among its corners (nine atomics per run
// of lanes whose corner sits in one cluster), its orientation (1 B) and its key (8 B).  An index outside [0, V) is never read through.
__global__ void __launch_bounds__(SIMP_BLOCK) simp_faces_kernel(const float* __restrict__ verts, const int* __restrict__ faces, int V,
                                                               int F, SBox bx, const int* __restrict__ vcid,
                                                               int64_t* __restrict__ acc, int64_t* __restrict__ keys,
                                                               uint8_t* __restrict__ par) {
  const int f = blockIdx.x * SIMP_BLOCK + threadIdx.x;
  int g[3] = {-1, -1, -1};
  bool ok = f < F;
  if (ok) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int v = faces[3 * f + c];
      g[c] = (v >= 0 && v < V) ? vcid[v] : -1;
      ok = ok && g[c] >= 0;
    }
  }
  double t[3][3], q[3][3];
  int slot[3] = {-1, -1, -1};                        // the cluster corner c adds this face's quadric to, -1: none
  if (ok) {
#pragma unroll
    for (int c = 0; c < 3; ++c) cell_of(verts, faces[3 * f + c], bx, t[c], q[c]);
    slot[0] = g[0];
    if (g[1] != g[0]) slot[1] = g[1];
    if (g[2] != g[0] && g[2] != g[1]) slot[2] = g[2];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (!__any(slot[c] >= 0)) continue;              // wave-uniform
    int64_t x[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (slot[c] >= 0) quadric_of(t, q[c], x);
    if (wave_run_sum(slot[c], x)) {
      int64_t* A = acc + (int64_t)slot[c] * SIMP_ACC + 10;
#pragma unroll
      for (int k = 0; k < 9; ++k) add64(A + k, x[k]);
    }
  }
  if (f >= F) return;
  int64_t key = SIMP_NO_KEY;
  int odd = 0;
  if (ok && g[0] != g[1] && g[1] != g[2] && g[0] != g[2]) {
    const int lo = min(g[0], min(g[1], g[2])), hi = max(g[0], max(g[1], g[2]));
    const int mid = (int)((int64_t)g[0] + g[1] + g[2] - lo - hi);
    key = ((int64_t)lo << (2 * SIMP_KEY_BITS)) | ((int64_t)mid << SIMP_KEY_BITS) | (int64_t)hi;
    odd = ((g[0] < g[1]) + (g[1] < g[2]) + (g[0] < g[2])) & 1;
  }
  keys[f] = key;
  par[f] = (uint8_t)odd;
}

// ---- runs on the sorted keys.  Position i heads a run when its key differs from its predecessor's; it is odd when its face is.
__device__ __forceinline__ void run_flags(const int64_t* __restrict__ keys, const int64_t* __restrict__ perm,
                                          const uint8_t* __restrict__ par, int F, int i, int* v) {
  v[0] = 0; v[1] = 0;
  if (i >= F) return;
  const int64_t k = keys[i];
  v[0] = i == 0 || keys[i - 1] != k;
  v[1] = k != SIMP_NO_KEY && par[perm[i]];
}
__global__ void __launch_bounds__(SIMP_BLOCK) simp_runs_count_kernel(const int64_t* __restrict__ keys, const int64_t* __restrict__ perm,
                                                                    const uint8_t* __restrict__ par, int F,
                                                                    int64_t* __restrict__ blk, int64_t nblk) {
  int v[2];
  run_flags(keys, perm, par, F, blockIdx.x * SIMP_BLOCK + threadIdx.x, v);
  int64_t t[2];
  block_sum<SIMP_BLOCK>({v[0], v[1]}, t);
  if (threadIdx.x == 0) {
    blk[blockIdx.x] = t[0];
    blk[nblk + blockIdx.x] = t[1];
  }
}
// per position its run and the odd faces below it; per run its first position; heads[runs] = odd[F] closes both lists
__global__ void __launch_bounds__(SIMP_BLOCK) simp_runs_write_kernel(const int64_t* __restrict__ keys, const int64_t* __restrict__ perm,
                                                                    const uint8_t* __restrict__ par, int F,
                                                                    const int64_t* __restrict__ blk, int64_t nblk,
                                                                    const int64_t* __restrict__ cnt, int* __restrict__ rid,
                                                                    int* __restrict__ heads, int* __restrict__ odd) {
  const int i = blockIdx.x * SIMP_BLOCK + threadIdx.x;
  int v[2];
  run_flags(keys, perm, par, F, i, v);
  int64_t o[2] = {blk[blockIdx.x], blk[nblk + blockIdx.x]};
  block_offset<SIMP_BLOCK>({v[0], v[1]}, o);
  if (i == 0) {
    heads[cnt[1]] = F;
    odd[F] = (int)cnt[2];
  }
  if (i >= F) return;
  const int r = (int)o[0] + v[0] - 1;                // heads at or below i, less one
  rid[i] = r;
  odd[i] = (int)o[1];
  if (v[0]) heads[r] = i;
}

// ---- survivors: in a run with p even and m odd faces the first min(p, m) of each orientation in input order (= sorted order:
// the sort is stable) go.  Constant work per position.  A survivor marks its three clusters.
__global__ void __launch_bounds__(SIMP_BLOCK) simp_survivors_kernel(const int64_t* __restrict__ keys, const int64_t* __restrict__ perm,
                                                                   const uint8_t* __restrict__ par, const int* __restrict__ faces, int F,
                                                                   const int* __restrict__ rid, const int* __restrict__ heads,
                                                                   const int* __restrict__ odd, const int* __restrict__ vcid,
                                                                   int V, int* __restrict__ keep, int* __restrict__ used) {
  const int i = blockIdx.x * SIMP_BLOCK + threadIdx.x;
  if (i >= F) return;
  const int64_t p = perm[i];
  if (p < 0 || p >= F) return;                       // not a permutation: write nothing through it
  const int f = (int)p;
  int k = 0, g[3];
  bool ok = keys[i] != SIMP_NO_KEY;
#pragma unroll
  for (int c = 0; c < 3; ++c) {                      // (a key that is not this face's: touch nothing through it)
    const int v = faces[3 * f + c];
    g[c] = (v >= 0 && v < V) ? vcid[v] : -1;
    ok = ok && g[c] >= 0;
  }
  if (ok) {
    const int r = rid[i], s = heads[r], e = heads[r + 1];
    const int m = odd[e] - odd[s], pe = (e - s) - m;
    const int below = odd[i] - odd[s];
    const int rank = par[f] ? below : (i - s) - below;
    k = rank >= min(pe, m);
  }
  keep[f] = k;
  if (!k) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) used[g[c]] = 1;       // every writer stores the same value
}

// (the two compactions' counts, used clusters over K_max slots with K from device memory and kept faces: scan.h's flag count)

// ---- solve: per used cluster its vertex (12 B), normal (12 B), colour (12 B) and colour query row (44 B), at its new id
__global__ void __launch_bounds__(SIMP_BLOCK) simp_solve_kernel(const int64_t* __restrict__ acc, const int* __restrict__ ckey,
                                                               const int* __restrict__ used, const int64_t* __restrict__ cnt,
                                                               const int64_t* __restrict__ blk, SBox bx, int quadric, int64_t V_out,
                                                               int* __restrict__ newid, float* __restrict__ verts,
                                                               float* __restrict__ normals, float* __restrict__ colors,
                                                               float* __restrict__ rows) {
  const int64_t K = cnt[0];
  const int64_t c = (int64_t)blockIdx.x * SIMP_BLOCK + threadIdx.x;
  const int u = c < K ? (used[c] != 0) : 0;
  const int64_t id = block_offset<SIMP_BLOCK>(u, blk[blockIdx.x]);
  if (c >= K) return;
  newid[c] = u ? (int)id : -1;
  if (!u || id >= V_out) return;
  const int64_t* A = acc + c * SIMP_ACC;
  const double n = (double)A[0];
  double ub[3], x[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) x[a] = ub[a] = (double)A[1 + a] / 4294967296.0 / n;
  if (quadric) {
    double Q[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) Q[k] = (double)A[10 + k] / 4294967296.0;
    double s[3];                                     // accepted inside its cell only
    if (quadric_solve(Q, ub, s) && isfinite(s[0]) && isfinite(s[1]) && isfinite(s[2]) && fabs(s[0]) <= 0.5 && fabs(s[1]) <= 0.5 &&
        fabs(s[2]) <= 0.5) {
      x[0] = s[0]; x[1] = s[1]; x[2] = s[2];
    }
  }
  const int key = ckey[c];
  const int G = bx.G;
  const double q[3] = {(double)(key % G), (double)((key / G) % G), (double)(key / (G * G))};
  const double s[3] = {(double)A[4] / 1073741824.0, (double)A[5] / 1073741824.0, (double)A[6] / 1073741824.0};
  const double len = sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
  float xo[3], no[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    xo[a] = (float)(bx.lo[a] + ((q[a] + 0.5) + x[a]) * bx.c[a]);
    no[a] = len > 0.0 ? (float)(s[a] / len) : 0.0f;
    verts[3 * id + a] = xo[a];
    normals[3 * id + a] = no[a];
    if (colors) colors[3 * id + a] = (float)((double)A[7 + a] / 1073741824.0 / n);
  }
  if (rows) write_color_row(rows, id, xo, no);
}

// ---- faces out: 4 + 12 B read per face, 12 B written per survivor, renumbered, in input order
__global__ void __launch_bounds__(SIMP_BLOCK) simp_faces_write_kernel(const int* __restrict__ faces, int F, const int* __restrict__ keep,
                                                                     const int64_t* __restrict__ blk, const int* __restrict__ vcid,
                                                                     const int* __restrict__ newid, int64_t F_out,
                                                                     int* __restrict__ out) {
  const int f = blockIdx.x * SIMP_BLOCK + threadIdx.x;
  const int k = f < F ? (keep[f] != 0) : 0;
  const int64_t id = block_offset<SIMP_BLOCK>(k, blk[blockIdx.x]);
  if (!k || id >= F_out) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) out[3 * id + c] = newid[vcid[faces[3 * f + c]]];
}

// the grid and the item counts: all that nerf_simplify_count takes
int simp_size_check(const char* who, int64_t V, int64_t F, int G) {
  NERF_TRY(lattice_res_check(who, G, "grid"));
  NERF_REQUIRE(V >= 0 && V <= MESH_MAX_ITEMS && F >= 0 && F <= MESH_MAX_ITEMS, NERF_E_SHAPE,
               "%s: need 0 <= V, F <= 2^24 (got %lld, %lld)", who, (long long)V, (long long)F);
  return NERF_OK;
}

int simp_check(const char* who, int64_t V, int64_t F, const float* lo, const float* hi, int G, SBox* bx) {
  NERF_TRY(simp_size_check(who, V, F, G));
  NERF_REQUIRE(lo && hi, NERF_E_NULL, "%s: NULL lo / hi", who);
  const int64_t cells = lattice_n3(G);
  NERF_REQUIRE((V < cells ? V : cells) <= (1ll << SIMP_KEY_BITS), NERF_E_SHAPE,
               "%s: min(V, grid^3) = %lld clusters do not fit %d bits", who, (long long)(V < cells ? V : cells), SIMP_KEY_BITS);
  NERF_TRY(box_check(who, lo, hi));
  for (int a = 0; a < 3; ++a) {
    const double ext = (double)hi[a] - (double)lo[a];
    bx->lo[a] = (double)lo[a];
    bx->inv[a] = (double)G / ext;
    bx->c[a] = ext / (double)G;
  }
  bx->G = G;
  return NERF_OK;
}

#define SIMP_LAUNCH(what, kernel, blocks, ...) NERF_LAUNCH(what, kernel, blocks, SIMP_BLOCK, st, __VA_ARGS__)

}  // namespace
}  // namespace nerf

using namespace nerf;

extern "C" int64_t nerf_simplify_workspace_bytes(int64_t V, int64_t F, int grid) {
  if (!lattice_res_ok(grid) || V < 0 || V > MESH_MAX_ITEMS || F < 0 || F > MESH_MAX_ITEMS) return -1;
  return simp_ws(nullptr, V, F, grid).bytes;
}

extern "C" int nerf_simplify_cluster(const float* verts, const float* normals, const float* colors, int64_t V, const int32_t* faces,
                                     int64_t F, const float* lo, const float* hi, int grid, void* workspace, int64_t* tri_keys,
                                     void* stream) {
  SBox bx;
  NERF_TRY(simp_check("nerf_simplify_cluster", V, F, lo, hi, grid, &bx));
  if (V == 0 || F == 0) return NERF_OK;
  NERF_REQUIRE(verts && normals && faces && workspace && tri_keys, NERF_E_NULL, "nerf_simplify_cluster: NULL pointer");
  const SimpWs w = simp_ws(workspace, V, F, grid);
  hipStream_t st = as_stream(stream);
  NERF_HIP("nerf_simplify_cluster", hipMemsetAsync(w.mask, 0, w.W * sizeof(u64), st));
  SIMP_LAUNCH("nerf_simplify_cluster (keys)", simp_keys_kernel, mesh_blocks(V, SIMP_BLOCK), verts, (int)V, bx, w.mask, w.vcid);
  SIMP_LAUNCH("nerf_simplify_cluster (word counts)", simp_words_count_kernel, w.nblk_w, (const u64*)w.mask, w.W, w.blk_w);
  NERF_TRY(scan_launch("nerf_simplify_cluster (scan of the words)", w.blk_w, w.nblk_w, w.cnt, st));
  SIMP_LAUNCH("nerf_simplify_cluster (word prefixes)", simp_words_write_kernel, w.nblk_w, (const u64*)w.mask, w.W,
              (const int64_t*)w.blk_w, w.wpre);
  SIMP_LAUNCH("nerf_simplify_cluster (zero)", simp_zero_kernel, grid_for(w.K_max * SIMP_ACC, SIMP_BLOCK), (const int64_t*)w.cnt, w.acc,
              w.used);
  SIMP_LAUNCH("nerf_simplify_cluster (vertices)", simp_vertices_kernel, mesh_blocks(V, SIMP_BLOCK), verts, normals, colors, (int)V, bx,
              (const u64*)w.mask, (const int*)w.wpre, w.vcid, w.ckey, w.acc);
  SIMP_LAUNCH("nerf_simplify_cluster (faces)", simp_faces_kernel, mesh_blocks(F, SIMP_BLOCK), verts, faces, (int)V, (int)F, bx,
              (const int*)w.vcid, w.acc, tri_keys, w.par);
  return NERF_OK;
}

extern "C" int nerf_simplify_count(const int64_t* sorted_keys, const int64_t* perm, int64_t V, const int32_t* faces, int64_t F,
                                   int grid, void* workspace, int64_t* totals, void* stream) {
  NERF_TRY(simp_size_check("nerf_simplify_count", V, F, grid));
  NERF_REQUIRE(totals, NERF_E_NULL, "nerf_simplify_count: NULL totals");
  if (V == 0 || F == 0) return zero_i64("nerf_simplify_count", totals, 3, stream);
  NERF_REQUIRE(sorted_keys && perm && faces && workspace, NERF_E_NULL, "nerf_simplify_count: NULL pointer");
  const SimpWs w = simp_ws(workspace, V, F, grid);
  hipStream_t st = as_stream(stream);
  const int n = (int)F;
  const uint8_t* par = w.par;
  SIMP_LAUNCH("nerf_simplify_count (runs)", simp_runs_count_kernel, w.nblk_f, sorted_keys, perm, par, n, w.blk_s, w.nblk_f);
  NERF_TRY(scan_launch("nerf_simplify_count (scan of the run heads)", w.blk_s, w.nblk_f, w.cnt + 1, st));
  NERF_TRY(scan_launch("nerf_simplify_count (scan of the odd faces)", w.blk_s + w.nblk_f, w.nblk_f, w.cnt + 2, st));
  SIMP_LAUNCH("nerf_simplify_count (run ranks)", simp_runs_write_kernel, w.nblk_f, sorted_keys, perm, par, n,
              (const int64_t*)w.blk_s, w.nblk_f, (const int64_t*)w.cnt, w.rid, w.heads, w.odd);
  SIMP_LAUNCH("nerf_simplify_count (survivors)", simp_survivors_kernel, w.nblk_f, sorted_keys, perm, par, faces, n,
              (const int*)w.rid, (const int*)w.heads, (const int*)w.odd, (const int*)w.vcid, (int)V, w.keep, w.used);
  SIMP_LAUNCH("nerf_simplify_count (used clusters)", scan_flags_count_kernel<SIMP_BLOCK>, w.nblk_c, (const int*)w.used,
              (const int64_t*)w.cnt, (int64_t)0, w.blk_c);
  NERF_TRY(scan_launch("nerf_simplify_count (scan of the clusters)", w.blk_c, w.nblk_c, totals, st));
  SIMP_LAUNCH("nerf_simplify_count (kept faces)", scan_flags_count_kernel<SIMP_BLOCK>, w.nblk_f, (const int*)w.keep,
              (const int64_t*)nullptr, F, w.blk_f);
  NERF_TRY(scan_launch("nerf_simplify_count (scan of the faces)", w.blk_f, w.nblk_f, totals + 1, st));
  NERF_HIP("nerf_simplify_count", hipMemcpyAsync(totals + 2, w.cnt, sizeof(int64_t), hipMemcpyDeviceToDevice, st));
  return NERF_OK;
}

extern "C" int nerf_simplify_write(int64_t V, const int32_t* faces, int64_t F, const float* lo, const float* hi, int grid,
                                   int placement, void* workspace, int64_t V_out, int64_t F_out, float* verts_out,
                                   float* normals_out, float* colors_out, float* color_rows, int32_t* faces_out, void* stream) {
  SBox bx;
  NERF_TRY(simp_check("nerf_simplify_write", V, F, lo, hi, grid, &bx));
  NERF_REQUIRE(placement == NERF_SIMPLIFY_MEAN || placement == NERF_SIMPLIFY_QUADRIC, NERF_E_SHAPE,
               "nerf_simplify_write: placement must be 0 (mean) or 1 (quadric), got %d", placement);
  NERF_REQUIRE(V_out >= 0 && V_out <= V && F_out >= 0 && F_out <= F, NERF_E_SHAPE,
               "nerf_simplify_write: bad V_out %lld / F_out %lld", (long long)V_out, (long long)F_out);
  if (V_out == 0 && F_out == 0) return NERF_OK;
  NERF_REQUIRE(faces && workspace && verts_out && normals_out && faces_out, NERF_E_NULL, "nerf_simplify_write: NULL pointer");
  const SimpWs w = simp_ws(workspace, V, F, grid);
  hipStream_t st = as_stream(stream);
  SIMP_LAUNCH("nerf_simplify_write (solve)", simp_solve_kernel, w.nblk_c, (const int64_t*)w.acc, (const int*)w.ckey,
              (const int*)w.used, (const int64_t*)w.cnt, (const int64_t*)w.blk_c, bx, placement, V_out, w.newid, verts_out,
              normals_out, colors_out, color_rows);
  SIMP_LAUNCH("nerf_simplify_write (faces)", simp_faces_write_kernel, w.nblk_f, faces, (int)F, (const int*)w.keep,
              (const int64_t*)w.blk_f, (const int*)w.vcid, (const int*)w.newid, F_out, faces_out);
  return NERF_OK;
}
