// Connected components of a thresholded density volume, and the filter that drops the small ones (the floaters of a trained
// field) before marching cubes.  Semantics in include/nerf_hip.h "connected components"; tests/_ccl_ref.py reproduces every
// output.  No reference counterpart.  Union-find in global memory with the smaller index winning (atomicMin on the parent
// array), so a component's root is its smallest linear index whatever the scheduling: every output is bit-reproducible.  The
// launch sequence depends on R alone and nothing is read on the host.  Every loop that follows parents or retries a union
// strictly lowers an index per iteration (parent[x] <= x throughout), so none can spin.  All HBM- or atomic-bound; bytes per
// voxel above each kernel.  Indexing, checks and the voxels of a workgroup: lattice.h.
#include "lattice.h"

namespace nerf {
namespace {

__device__ __forceinline__ int ld_parent(const int* parent, int x) {
  return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root above x: parents only ever fall (x -> parent[x] < x), so the walk ends after at most x steps.  A value that is not
// below x (x itself at a root; anything else cannot occur) ends it.
__device__ __forceinline__ int find_root(const int* parent, int x) {
  for (;;) {
    const int p = ld_parent(parent, x);
    if (p < 0 || p >= x) return x;
    x = p;
  }
}

// Joins the trees of a and b.  Per iteration: both are replaced by their roots, the larger root r is hung under the smaller one s
// with atomicMin.  If r was still a root (old == r) the trees are one.  Otherwise somebody hung r under old < r in between; the
// atomicMin has left parent[r] = min(old, s), and what remains is to join old and s: the pair's larger member fell strictly.
__device__ __forceinline__ void unite(int* parent, int a, int b) {
  const int a0 = a, b0 = b;
  for (;;) {
    a = find_root(parent, a);
    b = find_root(parent, b);
    if (a == b) break;
    const int r = a > b ? a : b, s = a > b ? b : a;
    const int old = atomicMin(parent + r, s);
    if (old == r) { a = s; break; }
    a = old;                                                   // old < r
    b = s;
  }
  // path compression of the two starting points: a is an ancestor of both by now (atomicMin never raises a parent)
  if (a < a0) atomicMin(parent + a0, a);
  if (a < b0) atomicMin(parent + b0, a);
}

// ---- init: 4 B of volume read, 4 B of parent written per voxel.  An inside voxel's parent is the first voxel of its run along x
// inside the workgroup (runs end at the row's end: i = R - 1 and the next row's i = 0 are adjacent in memory, not neighbours);
// an outside voxel's is -1.  Run starts by a max-scan over the workgroup's lanes.
__global__ void __launch_bounds__(LATTICE_BLOCK) ccl_init_kernel(const float* __restrict__ vol, int R, float iso, int* __restrict__ parent) {
  __shared__ int sh_in[LATTICE_BLOCK];
  __shared__ int sh_w[LATTICE_BLOCK / 64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t n3 = lattice_n3(R), lg = lattice_lane();
  const int l = (int)lg;
  const bool inside = lg < n3 && vol[lg < n3 ? l : 0] > iso;
  sh_in[tid] = inside ? 1 : 0;
  __syncthreads();
  const bool start = inside && (tid == 0 || l % R == 0 || !sh_in[tid - 1]);
  int x = start ? tid : -1;
  for (int o = 1; o < WAVE; o <<= 1) {
    const int t = __shfl_up(x, o, WAVE);
    if (lane >= o) x = max(x, t);
  }
  if (lane == 63) sh_w[w] = x;
  __syncthreads();
  for (int q = 0; q < w; ++q) x = max(x, sh_w[q]);
  if (lg < n3) parent[l] = inside ? (int)(lg - tid) + x : -1;
}

// ---- union: per inside voxel up to 7 volume values (cache hits) and, where the lattice does not already imply the join, one
// union with the neighbour below it along y and z (and along x across a workgroup's first voxel).  A join along y of p and
// q = p - R is implied when p - 1 and q - 1 are inside too: p ~ p - 1 and q ~ q - 1 along x, and p - 1 joins q - 1 itself (or
// hands it down the same way); along z likewise, through the x or the y neighbours.  On a solid region only its first
// row / column issues atomics.
__global__ void __launch_bounds__(LATTICE_BLOCK) ccl_union_kernel(const float* __restrict__ vol, int R, float iso, int* parent) {
  const int64_t n3 = lattice_n3(R), lg = lattice_lane();
  if (lg >= n3) return;
  const int l = (int)lg;
  if (!(vol[l] > iso)) return;
  int c[3];
  lattice_coords(l, R, c);
  const int sy = axis_stride(1, R), sz = axis_stride(2, R);
  const bool xm = c[0] > 0 && vol[l - 1] > iso;
  if (xm && threadIdx.x == 0) unite(parent, l, l - 1);
  const bool ym = c[1] > 0 && vol[l - sy] > iso;
  if (ym && !(xm && vol[l - sy - 1] > iso)) unite(parent, l, l - sy);
  if (c[2] > 0 && vol[l - sz] > iso) {
    const bool by_x = xm && vol[l - sz - 1] > iso;
    const bool by_y = ym && vol[l - sz - sy] > iso;
    if (!by_x && !by_y) unite(parent, l, l - sz);
  }
}

// ---- flatten: 4 B of parent read (plus the walk to the root, cache hits), 4 B of label written per voxel
__global__ void __launch_bounds__(LATTICE_BLOCK) ccl_flatten_kernel(const int* __restrict__ parent, int R, int* __restrict__ labels) {
  const int64_t n3 = lattice_n3(R), lg = lattice_lane();
  if (lg >= n3) return;
  int x = parent[lg];
  if (x >= 0) {
    for (;;) {
      const int p = parent[x];
      if (p < 0 || p >= x) break;
      x = p;
    }
  }
  labels[lg] = x;
}

// ---- sizes, 1 of 4: 4 B written per voxel; stats = 0
__global__ void __launch_bounds__(LATTICE_BLOCK) ccl_zero_kernel(int R, int* __restrict__ sizes, unsigned long long* __restrict__ stats) {
  const int64_t n3 = lattice_n3(R), lg = lattice_lane();
  if (lg < n3) sizes[lg] = 0;
  if (lg < 3) stats[lg] = 0ull;
}

// ---- sizes, 2 of 4: 4 B of label read per voxel; one integer atomic add per run of equal labels inside a wave (the run's
// length, from the ballot of the run heads), so a solid row costs one atomic per 64 voxels
__global__ void __launch_bounds__(LATTICE_BLOCK) ccl_count_kernel(const int* __restrict__ labels, int R, int* __restrict__ sizes) {
  const int lane = threadIdx.x & 63;
  const int64_t n3 = lattice_n3(R), lg = lattice_lane();
  const int lab = lg < n3 ? labels[lg] : -1;
  const int prev = __shfl_up(lab, 1, WAVE);
  const bool head = lane == 0 || prev != lab;
  const unsigned long long heads = __ballot(head);
  if (head && lab >= 0) {
    const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
    const int len = above ? __ffsll((long long)above) : 64 - lane;
    atomicAdd(sizes + lab, len);
  }
}

// ---- sizes, 3 of 4: 8 B read per voxel; per wave the roots, their voxels and the largest component's key
// (size << 32 | 0xFFFFFFFF - label: the most voxels, ties to the smaller label), then three 64-bit integer atomics per wave
__global__ void __launch_bounds__(LATTICE_BLOCK) ccl_roots_kernel(const int* __restrict__ labels, const int* __restrict__ sizes, int R,
                                                             unsigned long long* __restrict__ stats) {
  const int lane = threadIdx.x & 63;
  const int64_t n3 = lattice_n3(R), lg = lattice_lane();
  const bool root = lg < n3 && (int64_t)labels[lg < n3 ? lg : 0] == lg;
  const unsigned sz = root ? (unsigned)sizes[lg] : 0u;
  unsigned long long key = root ? ((unsigned long long)sz << 32) | (0xFFFFFFFFull - (unsigned long long)lg) : 0ull;
  unsigned long long vox = sz;
  const unsigned long long roots = __ballot(root);
  if (!roots) return;
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long t = __shfl_xor(key, o, WAVE);
    key = t > key ? t : key;
    vox += __shfl_xor(vox, o, WAVE);
  }
  if (lane == 0) {
    atomicAdd(stats + 0, (unsigned long long)__popcll(roots));
    atomicAdd(stats + 1, vox);
    atomicMax(stats + 2, key);
  }
}

// ---- sizes, 4 of 4: the key becomes the largest component's label, or -1 when there is none
__global__ void ccl_finish_kernel(int64_t* __restrict__ stats) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const unsigned long long key = (unsigned long long)stats[2];
    stats[2] = key ? (int64_t)(0xFFFFFFFFull - (key & 0xFFFFFFFFull)) : -1;
  }
}

// ---- filter: 4 + 4 B read (+ 4 B of size per inside voxel, cache hits on a large component), 4 B written per voxel.  Values
// move as bits (NaN payloads survive); out may be vol (each lane reads its voxel before it writes it).
__global__ void __launch_bounds__(LATTICE_BLOCK) ccl_filter_kernel(const uint32_t* vol, const int* __restrict__ labels,
                                                              const int* __restrict__ sizes, const int64_t* __restrict__ stats, int R,
                                                              uint32_t iso_bits, int64_t min_voxels, int largest_only, uint32_t* out) {
  const int64_t n3 = lattice_n3(R), lg = lattice_lane();
  if (lg >= n3) return;
  uint32_t v = vol[lg];
  const int lab = labels[lg];
  if (lab >= 0 && (int64_t)lab < n3) {
    bool drop = (int64_t)sizes[lab] < min_voxels;
    if (largest_only) drop = drop || (int64_t)lab != stats[2];
    if (drop) v = iso_bits;
  }
  out[lg] = v;
}

}  // namespace
}  // namespace nerf

using namespace nerf;

extern "C" int64_t nerf_ccl_workspace_bytes(int res) {
  return lattice_res_ok(res) ? lattice_n3(res) * (int64_t)sizeof(int32_t) : -1;
}

extern "C" int nerf_ccl_label(const float* vol, int res, float iso, void* workspace, int32_t* labels, void* stream) {
  const int rc = lattice_check("nerf_ccl_label", res, iso);
  if (rc) return rc;
  NERF_REQUIRE(vol && workspace && labels, NERF_E_NULL, "nerf_ccl_label: NULL pointer");
  int* parent = static_cast<int*>(workspace);
  const unsigned grid = lattice_blocks(res);
  hipStream_t st = as_stream(stream);
  NERF_LAUNCH("nerf_ccl_label (init)", ccl_init_kernel, grid, LATTICE_BLOCK, st, vol, res, iso, parent);
  NERF_LAUNCH("nerf_ccl_label (union)", ccl_union_kernel, grid, LATTICE_BLOCK, st, vol, res, iso, parent);
  NERF_LAUNCH("nerf_ccl_label (flatten)", ccl_flatten_kernel, grid, LATTICE_BLOCK, st, parent, res, labels);
  return NERF_OK;
}

extern "C" int nerf_ccl_sizes(const int32_t* labels, int res, int32_t* sizes, int64_t* stats, void* stream) {
  const int rc = lattice_res_check("nerf_ccl_sizes", res);
  if (rc) return rc;
  NERF_REQUIRE(labels && sizes && stats, NERF_E_NULL, "nerf_ccl_sizes: NULL pointer");
  unsigned long long* ustats = reinterpret_cast<unsigned long long*>(stats);
  const unsigned grid = lattice_blocks(res);
  hipStream_t st = as_stream(stream);
  NERF_LAUNCH("nerf_ccl_sizes (zero)", ccl_zero_kernel, grid, LATTICE_BLOCK, st, res, sizes, ustats);
  NERF_LAUNCH("nerf_ccl_sizes (count)", ccl_count_kernel, grid, LATTICE_BLOCK, st, labels, res, sizes);
  NERF_LAUNCH("nerf_ccl_sizes (roots)", ccl_roots_kernel, grid, LATTICE_BLOCK, st, labels, sizes, res, ustats);
  NERF_LAUNCH("nerf_ccl_sizes (finish)", ccl_finish_kernel, 1, 64, st, stats);
  return NERF_OK;
}

extern "C" int nerf_ccl_filter(const float* vol, const int32_t* labels, const int32_t* sizes, const int64_t* stats, int res, float iso,
                               int64_t min_voxels, int largest_only, float* out, void* stream) {
  const int rc = lattice_check("nerf_ccl_filter", res, iso);
  if (rc) return rc;
  NERF_REQUIRE(min_voxels >= 0, NERF_E_SHAPE, "nerf_ccl_filter: min_voxels must be >= 0 (got %lld)", (long long)min_voxels);
  NERF_REQUIRE(vol && labels && sizes && stats && out, NERF_E_NULL, "nerf_ccl_filter: NULL pointer");
  hipLaunchKernelGGL(ccl_filter_kernel, dim3(lattice_blocks(res)), dim3(LATTICE_BLOCK), 0, as_stream(stream),
                     reinterpret_cast<const uint32_t*>(vol), labels, sizes, stats, res, float_bits(iso), min_voxels, largest_only,
                     reinterpret_cast<uint32_t*>(out));
  return check_launch("nerf_ccl_filter");
}
