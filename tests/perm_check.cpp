// Stand-alone run of csrc/perm.h (host compiler, -fsanitize=address,undefined; run by tests/test_perm_host.py, which compares
// what this prints with ops.index.pixel_permutation_host).  Per domain in {1, 2, 35, 4096, 640 000, 2^33 + 5}, per seed: the key
// (half_bits, four round keys), then the values at offset + i for i < n = min(domain, 1000) at offset 0 and at offset domain - n;
// for the domains up to 4096 the run at offset 0 covers the whole domain.
#include <stdint.h>
#include <stdio.h>

#include "../nerf_meets_mlx_amd/csrc/perm.h"

using namespace nerf;

static void run(uint64_t domain, uint64_t seed, uint64_t offset, int64_t n, const PermKey& key) {
  printf("run %llu %llu %llu %lld\nv", (unsigned long long)domain, (unsigned long long)seed, (unsigned long long)offset, (long long)n);
  for (int64_t i = 0; i < n; ++i) printf(" %llu", (unsigned long long)perm_value(offset, i, domain, key));
  printf("\n");
}

int main() {
  const uint64_t domains[6] = {1, 2, 35, 4096, 640000, (1ull << 33) + 5};
  const uint64_t seeds[2] = {0, 0xFEDCBA9876543210ull};
  for (uint64_t domain : domains)
    for (uint64_t seed : seeds) {
      const PermKey key = make_key(seed, domain);
      printf("key %llu %llu %d %u %u %u %u\n", (unsigned long long)domain, (unsigned long long)seed, key.half_bits, key.k[0], key.k[1],
             key.k[2], key.k[3]);
      const int64_t n = domain < 1000 ? (int64_t)domain : 1000;
      run(domain, seed, 0, domain <= 4096 ? (int64_t)domain : n, key);
      run(domain, seed, domain - (uint64_t)n, n, key);
    }
  return 0;
}
