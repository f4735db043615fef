// Occupancy grid for empty-space skipping of the hash-grid model (Instant-NGP, Mueller et al. 2022, section 4): jittered cell
// points, the EMA-max merge of their density, the fixed-order threshold + bitfield pack, the stable cull / compaction of the samples
// of a batch, and the row scatter that puts the kept samples' outputs back.  No reference counterpart (include/nerf_hip.h).
// All of it is HBM- or launch-bound; each kernel's algorithmic bytes are in the comment above it.  No atomics anywhere: the
// compaction order comes from block scans, the mean from a fixed reduction tree, so every output is bit-reproducible.
#include "common.h"
#include "scan.h"

namespace nerf {
namespace {

constexpr int CULL_BLOCK = 256;                     // threads per cull workgroup
constexpr int CULL_ROUNDS = 4;                      // samples per thread: one block covers 1024 consecutive samples
constexpr int CULL_SPAN = CULL_BLOCK * CULL_ROUNDS;
constexpr int SUM_BLOCK = 256;                      // density mean: one partial per 4096 cells (16 per thread)
constexpr int SUM_SPAN = SUM_BLOCK * 16;

__host__ __device__ __forceinline__ uint64_t mix64(uint64_t z) {      // splitmix64 finaliser
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// cell of a unit-cube coordinate on one axis, or -1 when it lies outside [0, 1) (NaN included)
__device__ __forceinline__ int cell_1d(float u, float R) {
  if (!(u >= 0.0f && u < 1.0f)) return -1;
  const int c = (int)floorf(u * R);               // R a power of two: the product is exact
  return c;                                       // u < 1 and R * u exact: c <= R - 1
}

// the sample's cell index ix + R (iy + R iz), or -1 outside the box; the position is computed with exactly the roundings of the
// hash-grid kernels (hash_common.h point_of, mlp_input2.h ngp_row): (o + z d) * pos_scale + pos_offset, one rounding per op
__device__ __forceinline__ int64_t cell_of(const float* __restrict__ rr, float zv, float pos_scale, float pos_offset, int log2R) {
  const float R = (float)(1 << log2R);
  const int ix = cell_1d((rr[0] + zv * rr[3]) * pos_scale + pos_offset, R);
  const int iy = cell_1d((rr[1] + zv * rr[4]) * pos_scale + pos_offset, R);
  const int iz = cell_1d((rr[2] + zv * rr[5]) * pos_scale + pos_offset, R);
  if ((ix | iy | iz) < 0) return -1;
  return (int64_t)ix + ((int64_t)iy << log2R) + ((int64_t)iz << (2 * log2R));
}

__device__ __forceinline__ bool occupied(const uint32_t* __restrict__ bits, int64_t c) {
  return c >= 0 && ((bits[c >> 5] >> (c & 31)) & 1u);
}

// a kept sample: its depth (4 B) and its ray's row (44 B) at o
__device__ __forceinline__ void store_sample(float* rows_out, float* z_out, int64_t o, const float* rr, float zv) {
  z_out[o] = zv;
  float* dst = rows_out + o * NERF_RAY_STRIDE;
#pragma unroll
  for (int q = 0; q < NERF_RAY_STRIDE; ++q) dst[q] = rr[q];
}

// ---- jittered points: 44 + 4 B written per cell, nothing read.  Row = [p, d = 0, near = far = 0, viewdirs = 0], z = 0, so that
// nerf_ngp_query_fused_h evaluates the field at o + 0 * 0 = p exactly (n = 1).  d = 0 is harmless there: the kernel neither
// normalises d nor the view direction (sh_eval is a polynomial: SH of 0 is the constant band), near / far are not read, and sigma
// does not depend on the view branch of the 2 x 64 network.
__global__ void occ_points_kernel(int log2R, int64_t cell0, int64_t count, uint64_t key, float pos_scale, float pos_offset,
                                  float* __restrict__ rays, float* __restrict__ z) {
  const float R = (float)(1 << log2R), inv_R = 1.0f / R;
  const int64_t mask = (1ll << log2R) - 1;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c = cell0 + i;
    const int ci[3] = {(int)(c & mask), (int)((c >> log2R) & mask), (int)(c >> (2 * log2R))};
    float p[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const uint64_t h = mix64(key + (uint64_t)(3 * c + a + 1) * 0x9E3779B97F4A7C15ull);
      const float u = (float)(h >> 40) * 0x1p-24f;                 // [0, 1), 24 bits
      float q = ((float)ci[a] + u) * inv_R;
      p[a] = (q - pos_offset) / pos_scale;
      // the map back onto the unit cube rounds: a point it would move into a neighbour (or onto 1.0) goes to the cell centre
      if (cell_1d(p[a] * pos_scale + pos_offset, R) != ci[a]) {
        q = ((float)ci[a] + 0.5f) * inv_R;
        p[a] = (q - pos_offset) / pos_scale;
      }
    }
    float* r = rays + i * NERF_RAY_STRIDE;
    r[0] = p[0]; r[1] = p[1]; r[2] = p[2];
#pragma unroll
    for (int k = 3; k < NERF_RAY_STRIDE; ++k) r[k] = 0.0f;
    z[i] = 0.0f;
  }
}

// ---- merge: density = max(density * decay, relu(sigma)); 4 + 4 B read (sigma is one float of each 16-byte raw row, but the
// whole 64-byte line of 4 rows is fetched: 16 B per cell in practice), 4 B written per cell.
// NaN sigma counts as 0 (relu by `s > 0 ? s : 0`), so one NaN sample cannot poison the mean and with it the whole grid.
__global__ void occ_merge_kernel(float* __restrict__ density, const float* __restrict__ raw, int64_t count, float decay) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
    const float s = raw[4 * i + 3];
    const float r = s > 0.0f ? s : 0.0f;
    const float d = density[i] * decay;
    density[i] = r > d ? r : d;
  }
}

// ---- merge with the exp activation (the march mode's trunc_exp density): density = max(density * decay, exp(sigma)), NaN sigma
// counting as 0.  Same bytes as occ_merge_kernel.
__global__ void occ_merge_exp_kernel(float* __restrict__ density, const float* __restrict__ raw, int64_t count, float decay) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
    const float s = raw[4 * i + 3];
    const float r = (s == s) ? expf(s) : 0.0f;
    const float d = density[i] * decay;
    density[i] = r > d ? r : d;
  }
}

// fixed-order double sum of a block's values: per-thread partial (sequential), wave butterfly, then the waves in order
__device__ __forceinline__ double block_sum(double v, double* sh) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) sh[w] = v;
  __syncthreads();
  double t = 0.0;
  for (int k = 0; k < (int)(blockDim.x >> 6); ++k) t += sh[k];
  __syncthreads();
  return t;
}

// ---- mean, part 1: 4 B read per cell, 8 B written per 4096 cells.  Partial b = sum of cells [4096 b, 4096 (b + 1)) in double.
__global__ void __launch_bounds__(SUM_BLOCK) occ_partials_kernel(const float* __restrict__ density, int64_t ncells,
                                                                 double* __restrict__ partials) {
  __shared__ double sh[SUM_BLOCK / 64];
  const int64_t base = (int64_t)blockIdx.x * SUM_SPAN;
  double v = 0.0;
  for (int k = 0; k < SUM_SPAN / SUM_BLOCK; ++k) {
    const int64_t c = base + k * SUM_BLOCK + threadIdx.x;
    if (c < ncells) v += (double)density[c];
  }
  v = block_sum(v, sh);
  if (threadIdx.x == 0) partials[blockIdx.x] = v;
}

// ---- mean, part 2 + threshold + pack: every workgroup sums the same partials in the same order (8 B each, L2-resident), so all
// of them derive the same thr = min(thr_cap, float(sum / ncells)); then 4 B read per cell and 1 bit written.  Bit c of the field
// is bit (c & 31) of 32-bit word c >> 5: one wave ballot covers 64 consecutive cells = two words.
__global__ void __launch_bounds__(SUM_BLOCK) occ_pack_kernel(const float* __restrict__ density, int64_t ncells,
                                                             const double* __restrict__ partials, int nparts, float thr_cap,
                                                             uint32_t* __restrict__ bits, float* __restrict__ thr_out) {
  __shared__ double sh[SUM_BLOCK / 64];
  double v = 0.0;
  for (int k = threadIdx.x; k < nparts; k += SUM_BLOCK) v += partials[k];
  const double total = block_sum(v, sh);
  const float mean = (float)(total / (double)ncells);
  const float thr = mean < thr_cap ? mean : thr_cap;
  if (blockIdx.x == 0 && threadIdx.x == 0 && thr_out) *thr_out = thr;
  const int lane = threadIdx.x & 63;
  for (int64_t c0 = (int64_t)blockIdx.x * SUM_BLOCK; c0 < ncells; c0 += (int64_t)gridDim.x * SUM_BLOCK) {
    if (c0 + (threadIdx.x & ~63) >= ncells) break;          // ncells is a multiple of 64: whole waves in or out of range
    const int64_t c = c0 + threadIdx.x;
    const uint64_t m = __ballot(density[c] > thr);
    if (lane == 0) { bits[c >> 5] = (uint32_t)m; bits[(c >> 5) + 1] = (uint32_t)(m >> 32); }
  }
}

// ---- cull, pass 1: per workgroup of 1024 consecutive samples (ray-major: s = b n + j) the number kept; the raw rows of the culled
// samples get the (0, 0, 0, 0) fill.  Per sample: 4 B of z read, the ray's 24 B of o / d (shared by the n samples of a ray: cache
// hits), one bitfield word (the 256 KiB field of a 128^3 grid stays in L2), 16 B written when culled; 8 B per workgroup written.
__global__ void __launch_bounds__(CULL_BLOCK) occ_cull_count_kernel(const float* __restrict__ rays, const float* __restrict__ z,
                                                                    int64_t M, int n, const uint32_t* __restrict__ bits, int log2R,
                                                                    float pos_scale, float pos_offset, int64_t* __restrict__ counts,
                                                                    float* __restrict__ raw_fill) {
  int kept = 0;
  for (int k = 0; k < CULL_ROUNDS; ++k) {
    const int64_t s = (int64_t)blockIdx.x * CULL_SPAN + k * CULL_BLOCK + threadIdx.x;
    if (s >= M) continue;
    const bool keep = occupied(bits, cell_of(rays + (s / n) * NERF_RAY_STRIDE, z[s], pos_scale, pos_offset, log2R));
    kept += keep;
    if (!keep && raw_fill) reinterpret_cast<float4*>(raw_fill)[s] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
  const int64_t t = block_sum<CULL_BLOCK>(kept);
  if (threadIdx.x == 0) counts[blockIdx.x] = t;
}

// ---- cull, pass 2 (one workgroup): occ_cull_scan_kernel (scan.h).  8 + 8 B per 1024 samples.

// ---- cull, pass 3: the same keep decisions again (same reads as pass 1), their ranks inside the workgroup from wave ballots in
// sample order, and per kept sample: its index (8 B), its ray row (44 B) and depth (4 B) written at offset + rank.
__global__ void __launch_bounds__(CULL_BLOCK) occ_cull_compact_kernel(const float* __restrict__ rays, const float* __restrict__ z,
                                                                      int64_t M, int n, const uint32_t* __restrict__ bits, int log2R,
                                                                      float pos_scale, float pos_offset,
                                                                      const int64_t* __restrict__ offs, int64_t* __restrict__ idx_out,
                                                                      float* __restrict__ rays_out, float* __restrict__ z_out) {
  __shared__ int sh[CULL_BLOCK / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int64_t base = offs[blockIdx.x];
  for (int k = 0; k < CULL_ROUNDS; ++k) {
    const int64_t s = (int64_t)blockIdx.x * CULL_SPAN + k * CULL_BLOCK + threadIdx.x;
    const float* rr = rays + (s < M ? s / n : 0) * NERF_RAY_STRIDE;
    const float zv = s < M ? z[s] : 0.0f;
    const bool keep = s < M && occupied(bits, cell_of(rr, zv, pos_scale, pos_offset, log2R));
    const uint64_t m = __ballot(keep);
    if (lane == 0) sh[w] = __popcll(m);
    __syncthreads();
    int64_t before = base;
    for (int j = 0; j < w; ++j) before += sh[j];
    int64_t round_total = 0;
    for (int j = 0; j < CULL_BLOCK / 64; ++j) round_total += sh[j];
    if (keep) {
      const int64_t o = before + __popcll(m & ((1ull << lane) - 1ull));
      idx_out[o] = s;
      store_sample(rays_out, z_out, o, rr, zv);
    }
    base += round_total;
    __syncthreads();                                            // sh is rewritten by the next round
  }
}

// ---- occupancy-guided ray march (include/nerf_hip.h "ray march" spells out the arithmetic; tests/_march_ref.py reproduces it bit
// for bit).  One lane per ray.  The candidates of a ray are tested MARCH_GROUP at a time: their cells first, then the bitfield
// words of all of them in flight at once (independent L2 hits, ~200 cycles each, instead of one dependent hit per step), then
// the keep / stop decisions in order.  A candidate the decisions never reach is looked up for nothing; its cell is a valid index
// or -1, so every load stays inside the field.
constexpr int MARCH_BLOCK = 256;                    // rays per march workgroup
constexpr int MARCH_GROUP = 8;

// what a march is: the rays, their jitter (per ray, or one constant), the bitfield (NULL: every cell counts as occupied) and the
// step.  Filled by march_args on the host, passed by value to the four march kernels.
struct MarchArgs {
  const float* rays;
  int64_t B;
  const float* jitter;
  float jitter_const;
  const uint32_t* bits;
  int log2R;
  float pos_scale, pos_offset, step_world;
  int march_steps;
  __device__ __forceinline__ float jitter_of(int64_t b) const { return jitter ? jitter[b] : jitter_const; }
  __device__ __forceinline__ const float* row(int64_t b) const { return rays + b * NERF_RAY_STRIDE; }
};

struct MarchRay {
  // the ray's row, in registers: the kernels' pointers arrive inside MarchArgs, so without __restrict__, and a row read through
  // memory would be read again behind every store of a kept sample (and keep those stores from merging)
  float r[NERF_RAY_STRIDE];
  float t0, t1, dt, j;
  int kmax;                                         // 0: no sample (axis-parallel, NaN / inf, missed box)
};

__device__ __forceinline__ MarchRay march_setup(const MarchArgs& a, int64_t b) {
  const float jitter = a.jitter_of(b);
  MarchRay m;
#pragma unroll
  for (int q = 0; q < NERF_RAY_STRIDE; ++q) m.r[q] = a.row(b)[q];
  const float* rr = m.r;
  m.t0 = rr[6]; m.t1 = rr[7]; m.j = jitter; m.kmax = 0; m.dt = 0.0f;
  bool ok = isfinite(m.t0) && isfinite(m.t1) && isfinite(jitter);
#pragma unroll
  for (int x = 0; x < 6; ++x) ok = ok && isfinite(rr[x]);
  ok = ok && rr[3] != 0.0f && rr[4] != 0.0f && rr[5] != 0.0f;
  if (!ok) return m;
  const float lo = (0.0f - a.pos_offset) / a.pos_scale, hi = (1.0f - a.pos_offset) / a.pos_scale;      // the box, world units
#pragma unroll
  for (int x = 0; x < 3; ++x) {
    const float ta = (lo - rr[x]) / rr[3 + x], tb = (hi - rr[x]) / rr[3 + x];
    m.t0 = fmaxf(m.t0, fminf(ta, tb));
    m.t1 = fminf(m.t1, fmaxf(ta, tb));
  }
  // |d| through a double square root rounded once to float: the correctly rounded float square root, which the float
  // instruction sequence is not in every case
  const float dn = (float)sqrt((double)((rr[3] * rr[3] + rr[4] * rr[4]) + rr[5] * rr[5]));
  m.dt = a.step_world / dn;
  if (m.t0 < m.t1 && m.dt > 0.0f) m.kmax = 2 * a.march_steps;
  return m;
}

// Visits the kept samples of one ray in depth order: fn(i, z, row) for the i-th sample of this call.  The walk starts at candidate
// k_start with kept_start samples already kept (0 and 0: the whole march), and stops after max_new samples, at the cap of
// march_steps kept in all, or where the walk ends.  k_end = the candidate to resume at, or m.kmax when the ray has no candidate
// left.  Returns the number of samples visited.  RESUME = false (the one-shot march: 0, 0, march_steps) compiles the resume
// bookkeeping away, leaving k_end unset.
template <bool RESUME, class F>
__device__ __forceinline__ int march_ray(const MarchArgs& a, const MarchRay& m, int k_start, int kept_start, int max_new, int& k_end,
                                         F&& fn) {
  int kept = kept_start;
  if (RESUME) {
    k_end = m.kmax;
    if (kept >= a.march_steps) return 0;
  }
  for (int k0 = k_start; k0 < m.kmax; k0 += MARCH_GROUP) {
    float zs[MARCH_GROUP];
    int64_t cs[MARCH_GROUP];
    uint32_t ws[MARCH_GROUP];
#pragma unroll
    for (int g = 0; g < MARCH_GROUP; ++g) {
      zs[g] = m.t0 + ((float)(k0 + g) + m.j) * m.dt;
      cs[g] = cell_of(m.r, zs[g], a.pos_scale, a.pos_offset, a.log2R);
    }
#pragma unroll
    for (int g = 0; g < MARCH_GROUP; ++g) ws[g] = (a.bits && cs[g] >= 0) ? a.bits[cs[g] >> 5] : 0xFFFFFFFFu;
#pragma unroll
    for (int g = 0; g < MARCH_GROUP; ++g) {
      if (k0 + g >= m.kmax || !(zs[g] < m.t1)) return kept - kept_start;
      if (cs[g] >= 0 && ((ws[g] >> (cs[g] & 31)) & 1u)) {
        fn(kept - kept_start, zs[g], m.r);
        if (++kept == a.march_steps) return kept - kept_start;
        if (RESUME && kept - kept_start == max_new) {
          k_end = k0 + g + 1;
          return max_new;
        }
      }
    }
  }
  return kept - kept_start;
}

// the one-shot march of ray b: every kept sample to fn, their number back
template <class F>
__device__ __forceinline__ int march_whole(const MarchArgs& a, int64_t b, F&& fn) {
  int k_end;
  return march_ray<false>(a, march_setup(a, b), 0, 0, a.march_steps, k_end, fn);
}

// ---- march, pass 1: per ray the number of kept samples (int32 to the workspace), per workgroup of 256 rays their sum (int64).
// Per ray: 44 B of row read (the 32 B of o, d, near, far used), 4 B of jitter, one bitfield word per candidate (the 256 KiB field of
// a 128^3 grid: L2 hits, not HBM); 4 B written.
__global__ void __launch_bounds__(MARCH_BLOCK) occ_march_count_kernel(MarchArgs a, int* __restrict__ ray_counts,
                                                                      int64_t* __restrict__ blk) {
  const int64_t b = (int64_t)blockIdx.x * MARCH_BLOCK + threadIdx.x;
  int n = 0;
  if (b < a.B) ray_counts[b] = n = march_whole(a, b, [](int, float, const float*) {});
  const int64_t s = block_sum<MARCH_BLOCK>(n);
  if (threadIdx.x == 0) blk[blockIdx.x] = s;
}

// ---- march, pass 3 (pass 2 is occ_cull_scan_kernel over the workgroup sums): the ray's offset = its workgroup's offset + the
// exclusive scan of the counts inside the workgroup (8 B written), then the same march again, and per kept sample its ray row
// (44 B) and depth (4 B) written at offset + rank.  Reads as pass 1, plus 4 B of count per ray and 8 B per workgroup.
__global__ void __launch_bounds__(MARCH_BLOCK) occ_march_write_kernel(MarchArgs a, const int* __restrict__ ray_counts,
                                                                      const int64_t* __restrict__ blk, int64_t* __restrict__ offsets,
                                                                      float* __restrict__ rows_out, float* __restrict__ z_out) {
  const int64_t b = (int64_t)blockIdx.x * MARCH_BLOCK + threadIdx.x;
  const int n = b < a.B ? ray_counts[b] : 0;
  const int64_t base = block_offset<MARCH_BLOCK>(n, blk[blockIdx.x]);
  if (b >= a.B) return;
  offsets[b] = base;
  if (n == 0) return;
  march_whole(a, b, [&](int k, float zv, const float* rr) { store_sample(rows_out, z_out, base + k, rr, zv); });
}

// ---- resumed march of the round renderer (include/nerf_hip.h "early ray termination").  One lane per entry i of the live list;
// the ray b = live[i] resumes at its saved candidate and kept count (istate[b] = k, kept, samples, flags) and takes up to max_new
// further samples, each to fn.  It stays live when it took max_new and has candidates left; a ray the fold has terminated takes
// none.  Per entry: 4 B of live id, 16 B of state, the row (32 B used) and jitter, one bitfield word per candidate;
// entry = 2 n + live.
template <class F>
__device__ __forceinline__ int resume_ray(const MarchArgs& a, int b, const int* __restrict__ istate, int max_new, bool& more,
                                          int& k_end, F&& fn) {
  more = false;
  k_end = 0;
  if (b < 0 || b >= a.B || (istate[4 * b + 3] & NERF_ERT_TERMINATED)) return 0;
  const MarchRay m = march_setup(a, b);
  const int n = march_ray<true>(a, m, istate[4 * b], istate[4 * b + 1], max_new, k_end, fn);
  more = k_end < m.kmax;
  return n;
}

__global__ void __launch_bounds__(MARCH_BLOCK) ert_march_count_kernel(MarchArgs a, const int* __restrict__ live, int64_t A,
                                                                      const int* __restrict__ istate, int max_new,
                                                                      int* __restrict__ entry, int64_t* __restrict__ blk, int64_t nblk) {
  const int64_t i = (int64_t)blockIdx.x * MARCH_BLOCK + threadIdx.x;
  int n = 0;
  bool more = false;
  if (i < A) {
    int k_end;
    n = resume_ray(a, live[i], istate, max_new, more, k_end, [](int, float, const float*) {});
    entry[i] = 2 * n + (more ? 1 : 0);
  }
  int64_t t[2];
  block_sum<MARCH_BLOCK>({n, more ? 1 : 0}, t);
  if (threadIdx.x == 0) {
    blk[blockIdx.x] = t[0];
    blk[nblk + blockIdx.x] = t[1];
  }
}

// offsets[i] = the entry's sample offset, offsets[A] = K, the live rays in order to live_out, then the same walk again writing the
// rows (44 B) and depths (4 B), and the ray's resume point (8 B of state).  Reads as the count, plus 4 B of entry per ray.
__global__ void __launch_bounds__(MARCH_BLOCK) ert_march_write_kernel(MarchArgs a, const int* __restrict__ live, int64_t A,
                                                                      int* __restrict__ istate, int max_new,
                                                                      const int* __restrict__ entry, const int64_t* __restrict__ blk,
                                                                      int64_t nblk, int64_t* __restrict__ offsets,
                                                                      int* __restrict__ live_out, float* __restrict__ rows_out,
                                                                      float* __restrict__ z_out) {
  const int64_t i = (int64_t)blockIdx.x * MARCH_BLOCK + threadIdx.x;
  const int e = i < A ? entry[i] : 0;
  const int n = e >> 1, l = e & 1;
  int64_t off[2] = {blk[blockIdx.x], blk[nblk + blockIdx.x]};   // of the entry's samples, of its place in live_out
  block_offset<MARCH_BLOCK>({n, l}, off);
  if (i >= A) return;
  const int64_t base = off[0];
  offsets[i] = base;
  if (i == A - 1) offsets[A] = base + n;
  const int b = live[i];
  if (l) live_out[off[1]] = b;
  if (n == 0) return;
  bool more;
  int k_end;
  resume_ray(a, b, istate, max_new, more, k_end,
             [&](int k, float zv, const float* rr) { store_sample(rows_out, z_out, base + k, rr, zv); });
  istate[4 * b] = k_end;
  istate[4 * b + 1] += n;
}

// ---- dst[idx[i], :] = src[i, :]: 8 + 4 C B read, 4 C B written per row (C = 4: one float4 each way).
__global__ void scatter_rows_kernel(const float* __restrict__ src, const int64_t* __restrict__ idx, int64_t n, int C, int vec4,
                                    float* __restrict__ dst, int64_t n_dst) {
  if (vec4) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
      const int64_t r = idx[i];
      if (r >= 0 && r < n_dst) reinterpret_cast<float4*>(dst)[r] = reinterpret_cast<const float4*>(src)[i];
    }
    return;
  }
  const int64_t total = n * C;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t / C;
    const int c = (int)(t - i * C);
    const int64_t r = idx[i];
    if (r >= 0 && r < n_dst) dst[r * C + c] = src[t];
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int occ_res_check(const char* who, int log2_res) {
  NERF_REQUIRE(log2_res >= 2 && log2_res <= 10, NERF_E_SHAPE, "%s: need 2 <= log2_res <= 10", who);
  return NERF_OK;
}

int64_t march_blocks(int64_t n) { return (n + MARCH_BLOCK - 1) / MARCH_BLOCK; }
int64_t ray_ints(int64_t B) { return ((B * (int64_t)sizeof(int) + 7) / 8) * 8; }

// the workspaces of the two march pairs: blk[nblk], then one count per ray; and blk[2][nblk], then one entry per live ray.  The
// entries lie where the workspace of B rays puts them, whatever A <= B is; the two rows of blk are those of the launch (A).
PairWs march_ws(void* ws, int64_t B) { return pair_ws(ws, 1, march_blocks(B), ray_ints(B)); }
PairWs ert_ws(void* ws, int64_t B, int64_t A) {
  PairWs w = pair_ws(ws, 2, march_blocks(B), ray_ints(B));
  w.nblk = march_blocks(A);
  return w;
}

// The checks every march entry starts with, in this order (which fault wins is part of the behaviour), then the description the
// kernels take.  `offsets`: the entry's first output, whatever it calls it.
int march_args(const char* who, const float* rays, int64_t B, const float* jitter, float jitter_const, const uint32_t* bits,
               int log2_res, float pos_scale, float pos_offset, float step_world, int march_steps, void* workspace,
               int64_t* offsets, MarchArgs* a) {
  if (int rc = occ_res_check(who, log2_res)) return rc;
  NERF_REQUIRE(B >= 0 && B < (1ll << 40), NERF_E_SHAPE, "%s: bad B", who);
  NERF_REQUIRE(march_steps >= 1 && march_steps <= NERF_MARCH_MAX_STEPS, NERF_E_SHAPE, "%s: need 1 <= march_steps <= %d (got %d)",
               who, NERF_MARCH_MAX_STEPS, march_steps);
  NERF_REQUIRE(pos_scale != 0.0f && step_world > 0.0f, NERF_E_SHAPE, "%s: need pos_scale != 0 and step_world > 0", who);
  NERF_REQUIRE(offsets, NERF_E_NULL, "%s: NULL offsets", who);
  NERF_REQUIRE(B == 0 || (rays && workspace), NERF_E_NULL, "%s: NULL pointer", who);
  *a = MarchArgs{rays, B, jitter, jitter_const, bits, log2_res, pos_scale, pos_offset, step_world, march_steps};
  return NERF_OK;
}

// the early-termination entries' checks on top
int ert_march_check(const char* who, const MarchArgs& a, const int* live, int64_t A, const int* istate, int max_new) {
  NERF_REQUIRE(a.B < (1ll << 31) && A >= 0 && A <= a.B, NERF_E_SHAPE, "%s: need 0 <= A <= B < 2^31", who);
  NERF_REQUIRE(max_new >= 1, NERF_E_SHAPE, "%s: need max_new >= 1 (got %d)", who, max_new);
  NERF_REQUIRE(A == 0 || (live && istate), NERF_E_NULL, "%s: NULL live / istate", who);
  return NERF_OK;
}

}  // namespace
}  // namespace nerf

using namespace nerf;

extern "C" int64_t nerf_occ_finalize_workspace_bytes(int log2_res) {
  if (log2_res < 2 || log2_res > 10) return -1;
  const int64_t ncells = 1ll << (3 * log2_res);
  return ((ncells + SUM_SPAN - 1) / SUM_SPAN) * (int64_t)sizeof(double);
}

extern "C" int64_t nerf_occ_cull_workspace_bytes(int64_t B, int n) {
  if (B < 0 || n < 0) return -1;
  const int64_t M = B * (int64_t)n;
  return ((M + CULL_SPAN - 1) / CULL_SPAN) * (int64_t)sizeof(int64_t);
}

extern "C" int nerf_occ_points(int log2_res, int64_t cell0, int64_t count, uint64_t seed, uint64_t update, float pos_scale,
                               float pos_offset, float* rays_out, float* z_out, void* stream) {
  if (int rc = occ_res_check("nerf_occ_points", log2_res)) return rc;
  const int64_t ncells = 1ll << (3 * log2_res);
  NERF_REQUIRE(cell0 >= 0 && count >= 0 && cell0 + count <= ncells, NERF_E_SHAPE,
               "nerf_occ_points: cells [%lld, %lld) outside the grid of %lld", (long long)cell0, (long long)(cell0 + count),
               (long long)ncells);
  NERF_REQUIRE(pos_scale != 0.0f, NERF_E_SHAPE, "nerf_occ_points: pos_scale must be nonzero");
  if (count == 0) return NERF_OK;
  NERF_REQUIRE(rays_out && z_out, NERF_E_NULL, "nerf_occ_points: NULL pointer");
  const uint64_t key = mix64(seed ^ mix64(update + 0x632BE59BD9B4E019ull));
  hipLaunchKernelGGL(occ_points_kernel, dim3(grid_for(count, 256)), dim3(256), 0, as_stream(stream), log2_res, cell0, count, key,
                     pos_scale, pos_offset, rays_out, z_out);
  return check_launch("nerf_occ_points");
}

extern "C" int nerf_occ_merge(float* density, const float* raw, int64_t count, float decay, void* stream) {
  NERF_REQUIRE(count >= 0, NERF_E_SHAPE, "nerf_occ_merge: bad count");
  if (count == 0) return NERF_OK;
  NERF_REQUIRE(density && raw, NERF_E_NULL, "nerf_occ_merge: NULL pointer");
  hipLaunchKernelGGL(occ_merge_kernel, dim3(grid_for(count, 256)), dim3(256), 0, as_stream(stream), density, raw, count, decay);
  return check_launch("nerf_occ_merge");
}

extern "C" int nerf_occ_merge_ex(float* density, const float* raw, int64_t count, float decay, int activation, void* stream) {
  NERF_REQUIRE(count >= 0, NERF_E_SHAPE, "nerf_occ_merge_ex: bad count");
  NERF_REQUIRE(activation == NERF_OCC_RELU || activation == NERF_OCC_EXP, NERF_E_SHAPE,
               "nerf_occ_merge_ex: activation must be NERF_OCC_RELU (0) or NERF_OCC_EXP (1), got %d", activation);
  if (activation == NERF_OCC_RELU) return nerf_occ_merge(density, raw, count, decay, stream);
  if (count == 0) return NERF_OK;
  NERF_REQUIRE(density && raw, NERF_E_NULL, "nerf_occ_merge_ex: NULL pointer");
  hipLaunchKernelGGL(occ_merge_exp_kernel, dim3(grid_for(count, 256)), dim3(256), 0, as_stream(stream), density, raw, count, decay);
  return check_launch("nerf_occ_merge_ex");
}

extern "C" int nerf_occ_finalize(const float* density, int log2_res, float thr_cap, void* workspace, float* thr_out,
                                 uint32_t* bits, void* stream) {
  if (int rc = occ_res_check("nerf_occ_finalize", log2_res)) return rc;
  NERF_REQUIRE(density && workspace && bits, NERF_E_NULL, "nerf_occ_finalize: NULL pointer");
  const int64_t ncells = 1ll << (3 * log2_res);
  const int64_t nparts = (ncells + SUM_SPAN - 1) / SUM_SPAN;
  double* partials = static_cast<double*>(workspace);
  hipLaunchKernelGGL(occ_partials_kernel, dim3((unsigned)nparts), dim3(SUM_BLOCK), 0, as_stream(stream), density, ncells, partials);
  int rc = check_launch("nerf_occ_finalize (partial sums)");
  if (rc) return rc;
  hipLaunchKernelGGL(occ_pack_kernel, dim3(grid_for(ncells, SUM_BLOCK, 1024)), dim3(SUM_BLOCK), 0, as_stream(stream), density,
                     ncells, partials, (int)nparts, thr_cap, bits, thr_out);
  return check_launch("nerf_occ_finalize (pack)");
}

extern "C" int nerf_occ_cull(const float* rays, const float* z, int64_t B, int n, const uint32_t* bits, int log2_res,
                             float pos_scale, float pos_offset, void* workspace, int64_t* idx_out, int64_t* count_out,
                             float* rays_out, float* z_out, float* raw_fill, void* stream) {
  if (int rc = occ_res_check("nerf_occ_cull", log2_res)) return rc;
  NERF_REQUIRE(B >= 0 && n >= 0, NERF_E_SHAPE, "nerf_occ_cull: bad sizes");
  NERF_REQUIRE(count_out, NERF_E_NULL, "nerf_occ_cull: NULL count_out");
  const int64_t M = B * (int64_t)n;
  if (M == 0) return zero_i64("nerf_occ_cull", count_out, 1, stream);
  NERF_REQUIRE(rays && z && bits && workspace && idx_out && rays_out && z_out, NERF_E_NULL, "nerf_occ_cull: NULL pointer");
  NERF_REQUIRE(!raw_fill || aligned16(raw_fill), NERF_E_SHAPE, "nerf_occ_cull: raw_fill must be 16-byte aligned");
  const int64_t nblk = (M + CULL_SPAN - 1) / CULL_SPAN;
  NERF_REQUIRE(nblk < (1ll << 31), NERF_E_SHAPE, "nerf_occ_cull: B*n too large");
  int64_t* offs = static_cast<int64_t*>(workspace);
  hipLaunchKernelGGL(occ_cull_count_kernel, dim3((unsigned)nblk), dim3(CULL_BLOCK), 0, as_stream(stream), rays, z, M, n, bits,
                     log2_res, pos_scale, pos_offset, offs, raw_fill);
  int rc = check_launch("nerf_occ_cull (count)");
  if (rc) return rc;
  rc = scan_launch("nerf_occ_cull (scan)", offs, nblk, count_out, as_stream(stream));
  if (rc) return rc;
  hipLaunchKernelGGL(occ_cull_compact_kernel, dim3((unsigned)nblk), dim3(CULL_BLOCK), 0, as_stream(stream), rays, z, M, n, bits,
                     log2_res, pos_scale, pos_offset, offs, idx_out, rays_out, z_out);
  return check_launch("nerf_occ_cull (compact)");
}

extern "C" int64_t nerf_occ_march_workspace_bytes(int64_t B) { return B < 0 ? -1 : march_ws(nullptr, B).bytes; }

extern "C" int nerf_occ_march_count(const float* rays, int64_t B, const float* jitter, float jitter_const, const uint32_t* bits,
                                    int log2_res, float pos_scale, float pos_offset, float step_world, int march_steps,
                                    void* workspace, int64_t* offsets, void* stream) {
  MarchArgs a;
  int rc = march_args("nerf_occ_march_count", rays, B, jitter, jitter_const, bits, log2_res, pos_scale, pos_offset, step_world,
                      march_steps, workspace, offsets, &a);
  if (rc) return rc;
  if (B == 0) return zero_i64("nerf_occ_march_count", offsets, 1, stream);
  const PairWs w = march_ws(workspace, B);
  hipLaunchKernelGGL(occ_march_count_kernel, dim3((unsigned)w.nblk), dim3(MARCH_BLOCK), 0, as_stream(stream), a, w.items, w.blk);
  rc = check_launch("nerf_occ_march_count (count)");
  if (rc) return rc;
  return scan_launch("nerf_occ_march_count (scan)", w.blk, w.nblk, offsets + B, as_stream(stream));
}

extern "C" int nerf_occ_march_write(const float* rays, int64_t B, const float* jitter, float jitter_const, const uint32_t* bits,
                                    int log2_res, float pos_scale, float pos_offset, float step_world, int march_steps,
                                    void* workspace, int64_t* offsets, float* rows_out, float* z_out, void* stream) {
  MarchArgs a;
  int rc = march_args("nerf_occ_march_write", rays, B, jitter, jitter_const, bits, log2_res, pos_scale, pos_offset, step_world,
                      march_steps, workspace, offsets, &a);
  if (rc) return rc;
  if (B == 0) return NERF_OK;
  NERF_REQUIRE(rows_out && z_out, NERF_E_NULL, "nerf_occ_march_write: NULL rows_out / z_out");
  const PairWs w = march_ws(workspace, B);
  hipLaunchKernelGGL(occ_march_write_kernel, dim3((unsigned)w.nblk), dim3(MARCH_BLOCK), 0, as_stream(stream), a,
                     (const int*)w.items, (const int64_t*)w.blk, offsets, rows_out, z_out);
  return check_launch("nerf_occ_march_write");
}

extern "C" int nerf_scatter_rows(const float* src, const int64_t* idx, int64_t n, int channels, float* dst, int64_t n_dst,
                                 void* stream) {
  NERF_REQUIRE(n >= 0 && channels > 0 && n_dst >= 0, NERF_E_SHAPE, "nerf_scatter_rows: bad sizes");
  if (n == 0) return NERF_OK;
  NERF_REQUIRE(src && idx && dst, NERF_E_NULL, "nerf_scatter_rows: NULL pointer");
  const bool vec = channels == 4 && aligned16(src) && aligned16(dst);
  const int64_t items = vec ? n : n * channels;
  hipLaunchKernelGGL(scatter_rows_kernel, dim3(grid_for(items, 256)), dim3(256), 0, as_stream(stream), src, idx, n,
                     channels, (int)vec, dst, n_dst);
  return check_launch("nerf_scatter_rows");
}

extern "C" int64_t nerf_ert_march_workspace_bytes(int64_t B) { return B < 0 ? -1 : ert_ws(nullptr, B, B).bytes; }

extern "C" int nerf_ert_march_count(const float* rays, int64_t B, const float* jitter, float jitter_const, const uint32_t* bits,
                                    int log2_res, float pos_scale, float pos_offset, float step_world, int march_steps,
                                    const int* live, int64_t A, const int* istate, int max_new, void* workspace, int64_t* totals,
                                    void* stream) {
  MarchArgs a;
  int rc = march_args("nerf_ert_march_count", rays, B, jitter, jitter_const, bits, log2_res, pos_scale, pos_offset, step_world,
                      march_steps, workspace, totals, &a);
  if (!rc) rc = ert_march_check("nerf_ert_march_count", a, live, A, istate, max_new);
  if (rc) return rc;
  if (A == 0) return zero_i64("nerf_ert_march_count", totals, 2, stream);
  const PairWs w = ert_ws(workspace, B, A);
  hipLaunchKernelGGL(ert_march_count_kernel, dim3((unsigned)w.nblk), dim3(MARCH_BLOCK), 0, as_stream(stream), a, live, A, istate,
                     max_new, w.items, w.blk, w.nblk);
  rc = check_launch("nerf_ert_march_count (count)");
  if (rc) return rc;
  rc = scan_launch("nerf_ert_march_count (scan of the samples)", w.blk, w.nblk, totals, as_stream(stream));
  if (rc) return rc;
  return scan_launch("nerf_ert_march_count (scan of the live rays)", w.blk + w.nblk, w.nblk, totals + 1, as_stream(stream));
}

extern "C" int nerf_ert_march_write(const float* rays, int64_t B, const float* jitter, float jitter_const, const uint32_t* bits,
                                    int log2_res, float pos_scale, float pos_offset, float step_world, int march_steps,
                                    const int* live, int64_t A, int* istate, int max_new, void* workspace, int64_t* offsets,
                                    int* live_out, float* rows_out, float* z_out, void* stream) {
  MarchArgs a;
  int rc = march_args("nerf_ert_march_write", rays, B, jitter, jitter_const, bits, log2_res, pos_scale, pos_offset, step_world,
                      march_steps, workspace, offsets, &a);
  if (!rc) rc = ert_march_check("nerf_ert_march_write", a, live, A, istate, max_new);
  if (rc) return rc;
  if (A == 0) return zero_i64("nerf_ert_march_write", offsets, 1, stream);
  NERF_REQUIRE(live_out && rows_out && z_out, NERF_E_NULL, "nerf_ert_march_write: NULL live_out / rows_out / z_out");
  NERF_REQUIRE(live_out != live, NERF_E_SHAPE, "nerf_ert_march_write: live_out must not be live");
  const PairWs w = ert_ws(workspace, B, A);
  hipLaunchKernelGGL(ert_march_write_kernel, dim3((unsigned)w.nblk), dim3(MARCH_BLOCK), 0, as_stream(stream), a, live, A, istate,
                     max_new, (const int*)w.items, (const int64_t*)w.blk, w.nblk, offsets, live_out, rows_out, z_out);
  return check_launch("nerf_ert_march_write");
}
