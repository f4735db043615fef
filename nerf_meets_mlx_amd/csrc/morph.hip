// Morphological opening of a thresholded density volume ahead of the connected-component filter: an erosion that cuts the thin
// bridges between a floater and the surface, and the geodesic reconstruction that gives the kept pieces their skin back.
// Semantics in include/nerf_hip.h "morphological opening"; tests/_morph_ref.py reproduces every output.  No reference
// counterpart.  The radius-dependent work runs on bit-packed masks: a row along x is ceil(R / 64) 64-bit words, bit b of word wx
// is voxel i = 64 wx + b, the dead bits past i = R - 1 are always 0.  A y or z neighbour is then the same word of another row, an
// x neighbour a shift with one carry bit from the adjacent word of the same row (none across a row end).  A mask of R = 512 is
// 16 MiB against the volume's 512 MiB, so a step costs 1 / 32 of a float pass.  Launches: pack, r steps, apply -- (R, r) alone
// decide them, nothing is read on the host, and every output bit has one writer: bit-reproducible.
#include "lattice.h"
#define NERF_SCAN_HELPERS_ONLY                      // block_sum alone: this unit launches no scan and carves no pair workspace
#include "scan.h"

namespace nerf {
namespace {

constexpr int MORPH_BLOCK = LATTICE_BLOCK;         // voxels (pack, apply: lattice.h) or words (step) per workgroup, x fastest
constexpr int MORPH_STEP_MAX_BLOCKS = 1024;         // the steps stride over the words: at most 2 x 1024 atomics on the stats

typedef unsigned long long u64;

__host__ __device__ __forceinline__ int morph_row_words(int R) { return (R + 63) >> 6; }

// ---- pack: 4 B (8 B with seeds) read per voxel, 1 / 8 B written.  One wave per word: lane b holds voxel i = 64 wx + b of the row
// and the wave's ballot is the word; lanes past the row's end vote 0 (the dead bits).  With seeds: K = {kept > iso} within M.
// Also zeroes the two stats words for the steps' atomics.
template <bool SEEDS>
__global__ void __launch_bounds__(MORPH_BLOCK) morph_pack_kernel(const float* vol, const float* kept, int R, float iso,
                                                                u64* __restrict__ m_mask, u64* __restrict__ k_mask,
                                                                u64* __restrict__ stats) {
  const int lane = threadIdx.x & 63;
  const int W = morph_row_words(R);
  const int64_t n_words = (int64_t)W * R * R;
  const int64_t w = (int64_t)blockIdx.x * (MORPH_BLOCK / 64) + (threadIdx.x >> 6);
  if (blockIdx.x == 0 && threadIdx.x < 2) stats[threadIdx.x] = 0ull;
  if (w >= n_words) return;                          // wave-uniform
  const int wx = (int)(w % W);
  const int64_t row = w / W;
  const int i = wx * 64 + lane;
  const bool valid = i < R;
  const int64_t p = row * R + (valid ? i : 0);
  const bool in_m = valid && vol[p] > iso;
  const u64 m = __ballot(in_m);
  u64 k = 0ull;
  if (SEEDS) k = __ballot(in_m && kept[p] > iso);
  if (lane == 0) {
    m_mask[w] = m;
    if (SEEDS) k_mask[w] = k;
  }
}

// ---- step: one lane per word, striding; 7 words read (6 of them cache hits of the neighbouring lanes and rows), 1 written.
// Erosion: dst = src and its six neighbours, a neighbour beyond the lattice counting as outside.  Dilation: dst = (src or its six
// neighbours) within M.  count_src / count_dst (each may be NULL): the popcounts of src / dst, reduced over the workgroup, one
// integer atomic each per workgroup.
template <bool DILATE>
__global__ void __launch_bounds__(MORPH_BLOCK) morph_step_kernel(const u64* __restrict__ src, const u64* __restrict__ m_mask, int R,
                                                                u64* __restrict__ dst, u64* count_src, u64* count_dst) {
  const int W = morph_row_words(R);
  const int n_words = W * R * R;                     // <= 8 * 512 * 512
  const int sy = W, sz = W * R;
  int n_src = 0, n_dst = 0;                          // <= 64 * n_words < 2^31
  for (int w = blockIdx.x * MORPH_BLOCK + threadIdx.x; w < n_words; w += gridDim.x * MORPH_BLOCK) {
    const int wx = w % W, row = w / W;
    const int j = row % R, k = row / R;
    const u64 c = src[w];
    const u64 xm = (c << 1) | (wx > 0 ? src[w - 1] >> 63 : 0ull);          // bit b: voxel i - 1
    const u64 xp = (c >> 1) | (wx < W - 1 ? src[w + 1] << 63 : 0ull);      // bit b: voxel i + 1 (the dead bit past i = R - 1 is 0)
    const u64 ym = j > 0 ? src[w - sy] : 0ull;
    const u64 yp = j < R - 1 ? src[w + sy] : 0ull;
    const u64 zm = k > 0 ? src[w - sz] : 0ull;
    const u64 zp = k < R - 1 ? src[w + sz] : 0ull;
    const u64 d = DILATE ? (c | xm | xp | ym | yp | zm | zp) & m_mask[w] : c & xm & xp & ym & yp & zm & zp;
    dst[w] = d;
    n_src += __popcll(c);
    n_dst += __popcll(d);
  }
  if (!count_src && !count_dst) return;
  int64_t t[2];
  block_sum<MORPH_BLOCK>({n_src, n_dst}, t);
  if (threadIdx.x != 0) return;
  if (count_src && t[0]) atomicAdd(count_src, (u64)t[0]);
  if (count_dst && t[1]) atomicAdd(count_dst, (u64)t[1]);
}

// ---- apply: 4 B read, 4 B written per voxel (the two mask words of a wave's voxels are broadcast cache hits).  A voxel of M that
// is not in `keep` becomes iso; every other value moves as bits (NaN payloads survive).  out may be vol: each lane reads its voxel
// before it writes it.
__global__ void __launch_bounds__(LATTICE_BLOCK) morph_apply_kernel(const uint32_t* vol, const u64* __restrict__ m_mask,
                                                                 const u64* __restrict__ keep, int R, uint32_t iso_bits,
                                                                 uint32_t* out) {
  const int64_t lg = lattice_lane();
  if (lg >= lattice_n3(R)) return;
  const int W = morph_row_words(R);
  const int i = (int)(lg % R);
  const int64_t w = (lg / R) * W + (i >> 6);
  const u64 bit = 1ull << (i & 63);
  uint32_t v = vol[lg];
  if ((m_mask[w] & bit) && !(keep[w] & bit)) v = iso_bits;
  out[lg] = v;
}

int morph_check(const char* who, int R, float iso, int radius) {
  const int rc = lattice_check(who, R, iso);
  if (rc) return rc;
  NERF_REQUIRE(radius >= 1 && radius <= NERF_MORPH_MAX_RADIUS, NERF_E_SHAPE, "%s: need 1 <= radius <= %d (got %d)", who,
               NERF_MORPH_MAX_RADIUS, radius);
  return NERF_OK;
}

int64_t morph_words(int R) { return (int64_t)morph_row_words(R) * R * R; }

// the r steps from buf[a] to buf[a ^ 1] and back (buf[0], buf[1]: the ping-pong pair; the first step reads `first`); the first
// step counts its source into stats[0], the last its result into stats[1].  Returns the buffer that holds the result.
template <bool DILATE>
int morph_steps(const char* who, const u64* first, const u64* m_mask, u64* const buf[2], int into, int R, int radius, u64* stats,
                hipStream_t st, const u64** result) {
  const int grid = grid_for(morph_words(R), MORPH_BLOCK, MORPH_STEP_MAX_BLOCKS);
  const u64* src = first;
  for (int n = 0; n < radius; ++n) {
    u64* dst = buf[into];
    NERF_LAUNCH(who, morph_step_kernel<DILATE>, grid, MORPH_BLOCK, st, src, m_mask, R, dst, n == 0 ? stats + 0 : (u64*)nullptr,
                n == radius - 1 ? stats + 1 : (u64*)nullptr);
    src = dst;
    into ^= 1;
  }
  *result = src;
  return NERF_OK;
}

unsigned morph_pack_blocks(int R) { return (unsigned)((morph_words(R) + MORPH_BLOCK / 64 - 1) / (MORPH_BLOCK / 64)); }

}  // namespace
}  // namespace nerf

using namespace nerf;

// three masks: M and the ping-pong pair
extern "C" int64_t nerf_morph_workspace_bytes(int res) {
  return lattice_res_ok(res) ? 3 * morph_words(res) * (int64_t)sizeof(u64) : -1;
}

extern "C" int nerf_morph_erode(const float* vol, int res, float iso, int radius, void* workspace, float* core, int64_t* stats2,
                                void* stream) {
  int rc = morph_check("nerf_morph_erode", res, iso, radius);
  if (rc) return rc;
  NERF_REQUIRE(vol && workspace && core && stats2, NERF_E_NULL, "nerf_morph_erode: NULL pointer");
  const int64_t nw = morph_words(res);
  u64* m_mask = static_cast<u64*>(workspace);
  u64* const buf[2] = {m_mask + nw, m_mask + 2 * nw};
  u64* stats = reinterpret_cast<u64*>(stats2);
  hipStream_t st = as_stream(stream);
  NERF_LAUNCH("nerf_morph_erode (pack)", morph_pack_kernel<false>, morph_pack_blocks(res), MORPH_BLOCK, st, vol,
              (const float*)nullptr, res, iso, m_mask, (u64*)nullptr, stats);
  const u64* eroded = nullptr;
  rc = morph_steps<false>("nerf_morph_erode (step)", m_mask, m_mask, buf, 0, res, radius, stats, st, &eroded);
  if (rc) return rc;
  hipLaunchKernelGGL(morph_apply_kernel, dim3(lattice_blocks(res)), dim3(LATTICE_BLOCK), 0, st,
                     reinterpret_cast<const uint32_t*>(vol), m_mask, eroded, res, float_bits(iso), reinterpret_cast<uint32_t*>(core));
  return check_launch("nerf_morph_erode (apply)");
}

extern "C" int nerf_morph_reconstruct(const float* vol, const float* kept, int res, float iso, int radius, void* workspace, float* out,
                                      int64_t* stats2, void* stream) {
  int rc = morph_check("nerf_morph_reconstruct", res, iso, radius);
  if (rc) return rc;
  NERF_REQUIRE(vol && kept && workspace && out && stats2, NERF_E_NULL, "nerf_morph_reconstruct: NULL pointer");
  const int64_t nw = morph_words(res);
  u64* m_mask = static_cast<u64*>(workspace);
  u64* const buf[2] = {m_mask + nw, m_mask + 2 * nw};
  u64* stats = reinterpret_cast<u64*>(stats2);
  hipStream_t st = as_stream(stream);
  NERF_LAUNCH("nerf_morph_reconstruct (pack)", morph_pack_kernel<true>, morph_pack_blocks(res), MORPH_BLOCK, st, vol, kept, res, iso,
              m_mask, buf[0], stats);
  const u64* grown = nullptr;
  rc = morph_steps<true>("nerf_morph_reconstruct (step)", buf[0], m_mask, buf, 1, res, radius, stats, st, &grown);
  if (rc) return rc;
  hipLaunchKernelGGL(morph_apply_kernel, dim3(lattice_blocks(res)), dim3(LATTICE_BLOCK), 0, st,
                     reinterpret_cast<const uint32_t*>(vol), m_mask, grown, res, float_bits(iso), reinterpret_cast<uint32_t*>(out));
  return check_launch("nerf_morph_reconstruct (apply)");
}
