// The three passes shared by the compactions of occupancy.hip (cull, march, early termination), mesh.hip (marching cubes),
// morph.hip (the steps' statistics) and the mesh surface units (simplify.hip, decimate.hip, smooth.hip, distance.hip): count per
// workgroup (block_sum), scan of the workgroup sums by one workgroup (occ_cull_scan_kernel, launched by scan_launch), rank inside
// the workgroup (block_offset).  Fixed order, no atomics; the host's layout of the workspace a count / write pair shares; and,
// as templates that a unit emits only when it launches them, the two count / write forms that do the same work per item wherever
// they are used: counts to offsets (smooth.hip's rows, distance.hip's cells) and the count of set flags (simplify.hip, decimate.hip).
#pragma once
#include <type_traits>
#include "common.h"

namespace nerf {
namespace {

// Both helpers below contain a __syncthreads(): EVERY lane of the workgroup must reach them, lanes past the end of the data
// included (with v = 0), and none may have returned before.  BLOCK = the workgroup's threads; N counters of type T (int, or int64_t
// for distance.hip's weights) are carried at once.

// total[c] = the sum of v[c] over the workgroup in thread 0 (0 in every other): wave butterfly, lane 0 to LDS, thread 0 adds the waves.
template <int BLOCK, int N, class T = int>
__device__ __forceinline__ void block_sum(const T (&v)[N], int64_t (&total)[N]) {
  __shared__ T sh[N][BLOCK / WAVE];
  T t[N];
#pragma unroll
  for (int c = 0; c < N; ++c) t[c] = v[c];
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int c = 0; c < N; ++c) t[c] += __shfl_xor(t[c], o, WAVE);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int c = 0; c < N; ++c) sh[c][threadIdx.x >> 6] = t[c];
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < N; ++c) {
    total[c] = 0;
    if (threadIdx.x != 0) continue;
    for (int k = 0; k < BLOCK / WAVE; ++k) total[c] += sh[c][k];
  }
}

// off[c] += the exclusive prefix of v[c] over the workgroup's lanes in thread order (off[c] comes in as the workgroup's base):
// inclusive wave scan, last lane to LDS, the waves below added in order.
template <int BLOCK, int N, class T = int>
__device__ __forceinline__ void block_offset(const T (&v)[N], int64_t (&off)[N]) {
  __shared__ T sh[N][BLOCK / WAVE];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  T x[N];
#pragma unroll
  for (int c = 0; c < N; ++c) x[c] = v[c];
  for (int o = 1; o < WAVE; o <<= 1) {
#pragma unroll
    for (int c = 0; c < N; ++c) {
      const T t = __shfl_up(x[c], o, WAVE);
      if (lane >= o) x[c] += t;
    }
  }
  if (lane == 63) {
#pragma unroll
    for (int c = 0; c < N; ++c) sh[c][w] = x[c];
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < N; ++c) {
    off[c] += x[c] - v[c];
    for (int k = 0; k < w; ++k) off[c] += sh[c][k];
  }
}

// the one-counter forms (T is named, never deduced: an argument of another type converts to it)
template <int BLOCK, class T = int>
__device__ __forceinline__ int64_t block_sum(std::common_type_t<T> v) {
  int64_t t[1];
  block_sum<BLOCK, 1, T>({v}, t);
  return t[0];
}
template <int BLOCK, class T = int>
__device__ __forceinline__ int64_t block_offset(std::common_type_t<T> v, int64_t base) {
  int64_t o[1] = {base};
  block_offset<BLOCK, 1, T>({v}, o);
  return o[0];
}

// ---- counts -> exclusive offsets: count (the sum of cnt over each workgroup of BLOCK items) and, behind the scan of those sums,
// write (ranked inside the workgroup).  The write leaves the first slot of item i in off[i] and in cur[i], the fill cursor that held
// the count, and the total in off[n]; offsets and total are clamped at cap, not wrapped (a caller whose total can pass it refuses
// before anything reads them), and the unclamped total goes to total_out when that is not NULL.
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK) scan_offsets_count_kernel(const int* __restrict__ cnt, int n, int64_t* __restrict__ blk) {
  const int i = blockIdx.x * BLOCK + threadIdx.x;
  const int64_t t = block_sum<BLOCK>(i < n ? cnt[i] : 0);
  if (threadIdx.x == 0) blk[blockIdx.x] = t;
}
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK) scan_offsets_write_kernel(int* __restrict__ cur, int n, const int64_t* __restrict__ blk,
                                                                  const int64_t* __restrict__ total, int64_t cap,
                                                                  int* __restrict__ off, int64_t* __restrict__ total_out) {
  const int i = blockIdx.x * BLOCK + threadIdx.x;
  const int64_t o = block_offset<BLOCK>(i < n ? cur[i] : 0, blk[blockIdx.x]);
  if (i == 0) {
    const int64_t tot = total[0];
    off[n] = (int)(tot < cap ? tot : cap);
    if (total_out) total_out[0] = tot;
  }
  if (i >= n) return;
  const int oc = (int)(o < cap ? o : cap);
  off[i] = oc;
  cur[i] = oc;
}

// ---- the count of a compaction by flags: the items with flags[i] != 0 per workgroup, over n_dev[0] items, or n_host with n_dev NULL
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK) scan_flags_count_kernel(const int* __restrict__ flags, const int64_t* __restrict__ n_dev,
                                                                int64_t n_host, int64_t* __restrict__ blk) {
  const int64_t n = n_dev ? n_dev[0] : n_host;
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  const int64_t t = block_sum<BLOCK>(i < n ? (flags[i] != 0) : 0);
  if (threadIdx.x == 0) blk[blockIdx.x] = t;
}

#ifndef NERF_SCAN_HELPERS_ONLY                      // (a kernel defined here is emitted by every unit that includes it)
// counts -> exclusive offsets in place, the total to count_out.  8 + 8 B per count.
__global__ void __launch_bounds__(1024) occ_cull_scan_kernel(int64_t* __restrict__ offs, int64_t nblk, int64_t* __restrict__ count_out) {
  __shared__ int64_t sh[1024 / 64];
  __shared__ int64_t carry_sh;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int64_t carry = 0;
  for (int64_t b0 = 0; b0 < nblk; b0 += 1024) {
    const int64_t b = b0 + threadIdx.x;
    const int64_t v = b < nblk ? offs[b] : 0;
    int64_t x = v;                                               // inclusive wave scan
    for (int o = 1; o < WAVE; o <<= 1) {
      const int64_t t = __shfl_up(x, o, WAVE);
      if (lane >= o) x += t;
    }
    if (lane == 63) sh[w] = x;
    __syncthreads();
    int64_t before = carry;
    for (int k = 0; k < w; ++k) before += sh[k];
    if (b < nblk) offs[b] = before + x - v;
    if (threadIdx.x == 1023) carry_sh = before + x;
    __syncthreads();
    carry = carry_sh;
    __syncthreads();
  }
  if (threadIdx.x == 0) *count_out = carry;
}
inline int scan_launch(const char* what, int64_t* blk, int64_t nblk, int64_t* total, hipStream_t st) {
  hipLaunchKernelGGL(occ_cull_scan_kernel, dim3(1), dim3(1024), 0, st, blk, nblk, total);
  return check_launch(what);
}

// The workspace of a count / write pair: `rows` x nblk workgroup sums (int64, scanned in place), then item_bytes of one int per
// item.  The count entry, the write entries and the *_workspace_bytes function of a pair all take their pointers and sizes here.
struct PairWs {
  int64_t nblk;
  int64_t* blk;                                     // [rows][nblk]
  int* items;
  int64_t bytes;
};
inline PairWs pair_ws(void* ws, int rows, int64_t nblk, int64_t item_bytes) {
  const int64_t head = rows * nblk * (int64_t)sizeof(int64_t);
  return {nblk, static_cast<int64_t*>(ws), reinterpret_cast<int*>(reinterpret_cast<uintptr_t>(ws) + (uintptr_t)head), head + item_bytes};
}

// "nothing to do": n int64 zeros on the stream, or HIP's text
inline int zero_i64(const char* who, int64_t* p, int n, void* stream) {
  NERF_HIP(who, hipMemsetAsync(p, 0, n * sizeof(int64_t), as_stream(stream)));
  return NERF_OK;
}

#endif

}  // namespace
}  // namespace nerf
