// The block scan shared by the compactions of occupancy.hip (cull, march, early termination) and mesh.hip (marching cubes):
// one workgroup turns per-workgroup counts into exclusive offsets in place, in a fixed order (no atomics).
#pragma once
#include "common.h"

namespace nerf {
namespace {

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

}  // namespace
}  // namespace nerf
