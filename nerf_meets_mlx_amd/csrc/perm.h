// The keyed bijection of [0, domain) behind nerf_pixel_permutation and nerf_sample_batch (rays.hip): balanced Feistel on
// 2 * half_bits bits + cycle walking.  Host mirror: nerf_meets_mlx_amd/ops/index.py (must stay bit-identical).
// Compiles without HIP (tests/perm_check.cpp runs it under a host compiler).
#pragma once
#include <stdint.h>
#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

namespace nerf {

struct PermKey { uint32_t k[4]; int half_bits; };

__host__ __device__ inline uint32_t mix32(uint32_t x) {   // murmur3 finaliser
  x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
  return x;
}
__host__ __device__ inline uint64_t feistel(uint64_t v, const PermKey& key) {
  const uint32_t mask = (key.half_bits >= 32) ? 0xFFFFFFFFu : ((1u << key.half_bits) - 1u);
  uint32_t L = (uint32_t)(v >> key.half_bits) & mask, R = (uint32_t)v & mask;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    uint32_t f = mix32(R * 0x9E3779B1u + key.k[r]) & mask;
    uint32_t nl = R; R = L ^ f; L = nl;
  }
  return ((uint64_t)L << key.half_bits) | R;
}
static inline uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
// the smallest even number of bits (at least 2) that holds domain - 1, halved; four round keys from the seed
static inline PermKey make_key(uint64_t seed, uint64_t domain) {
  int bits = 2;
  while (bits < 64 && (1ull << bits) < domain) ++bits;
  if (bits & 1) ++bits;
  PermKey key;
  key.half_bits = bits / 2;
  for (int r = 0; r < 4; ++r) key.k[r] = (uint32_t)splitmix64(seed + (uint64_t)r);
  return key;
}
// the permutation's value at offset + i
__host__ __device__ inline uint64_t perm_value(uint64_t offset, int64_t i, uint64_t domain, const PermKey& key) {
  uint64_t v = offset + (uint64_t)i;
  do { v = feistel(v, key); } while (v >= domain);        // every cycle of P re-enters [0,domain)
  return v;
}

}  // namespace nerf
