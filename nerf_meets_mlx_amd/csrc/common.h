// Shared helpers for the gfx950 kernels behind include/nerf_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <mutex>
#include <type_traits>
#include <utility>

#include "../../include/nerf_hip.h"

#define WAVE 64

namespace nerf {

// last-error text (thread-compatible, one process per GPU)
char* err_buf();
int fail(int code, const char* fmt, ...);
int check_launch(const char* what);

static inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// One-time host set-up per DEVICE (the opt-in to dynamic LDS above 64 KiB: hipFuncSetAttribute applies to the device that is
// current when it is called, and a process may move between devices).  Thread-safe: std::call_once -- a second thread
// launching the same kernel returns from run() only after the first one's attribute call has completed (a plain bool flag set
// before / after the call let it launch in between).
struct DevOnce {
  std::once_flag flag[64];
  static int device() {
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) d = 0;
    return d;
  }
  template <class F> void run(int d, F&& f) { std::call_once(flag[d], std::forward<F>(f)); }     // d: device()
  template <class F> void run(F&& f) { run(device(), std::forward<F>(f)); }
};

// grid sizing for HBM-bound kernels: enough workgroups to fill 256 CUs, grid-stride the rest
static inline int grid_for(int64_t work_items, int block, int max_blocks = 256 * 8) {
  int64_t g = (work_items + block - 1) / block;
  if (g < 1) g = 1;
  if (g > max_blocks) g = max_blocks;
  return (int)g;
}
// the kernels with one wave per ray: four rays per 256-thread workgroup, at most max_blocks workgroups striding over the rest
static inline int wave_per_ray_grid(int64_t B, int max_blocks = 8192) { return grid_for(B, 4, max_blocks); }

// A runtime bool as a template argument: fn receives std::true_type / std::false_type, and a generic lambda names the
// kernel instantiation with decltype(arg)::value.  Nested calls list every combination once, in one place.  Returns what fn returns.
template <class Fn> static inline auto with_bool(bool b, Fn&& fn) { if (b) return fn(std::true_type{}); else return fn(std::false_type{}); }
// A runtime int as a template argument: fn receives std::integral_constant<int, V> for the first V of the list with v <= V
// (the last one if there is none).  Returns what fn returns.
template <int V, int... Vs, class Fn> static inline auto with_int_up_to(int v, Fn&& fn) {
  if constexpr (sizeof...(Vs) > 0) { if (v > V) return with_int_up_to<Vs...>(v, std::forward<Fn>(fn)); }
  return fn(std::integral_constant<int, V>{});
}

// ---- wave64 scans / reductions.  float: DPP (v_add_f32 ... row_shr / row_shl / row_bcast: the data path of the
// VALU, no LDS crossbar round trip per step as with ds_bpermute shuffles); double: shuffles (the one double scan,
// the importance sampler's CDF, must keep its summation order: its result is compared bit for bit with torch-CPU's).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_or_zero(float v) {          // lanes without a source (and masked rows) read 0.0f
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, false));
}
// inclusive prefix sum across the 64 lanes: Hillis-Steele inside each row of 16 (row_shr 1, 2, 4, 8), then the last lane
// of row 0 / 2 into rows 1 / 3 (row_bcast:15), then lane 31 into rows 2 and 3 (row_bcast:31)
__device__ __forceinline__ float wave_scan_incl(float v, int lane) {
  (void)lane;
  v += dpp_or_zero<0x111, 0xf>(v);
  v += dpp_or_zero<0x112, 0xf>(v);
  v += dpp_or_zero<0x114, 0xf>(v);
  v += dpp_or_zero<0x118, 0xf>(v);
  v += dpp_or_zero<0x142, 0xa>(v);
  v += dpp_or_zero<0x143, 0xc>(v);
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, wave_scan_incl(v, 0)), 63));
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
  return v;
}
// inclusive prefix sum across the 64 lanes (double: shuffles, see above)
__device__ __forceinline__ double wave_scan_incl(double v, int lane) {
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) {
    double t = __shfl_up(v, o, WAVE);
    if (lane >= o) v += t;
  }
  return v;
}
// inclusive suffix sum (lane i gets the sum over lanes >= i): row_shl 1, 2, 4, 8 inside each row of 16, then the totals of
// the rows above (they sit in the first lane of each row: three v_readlane) are added per row
__device__ __forceinline__ float wave_rscan_incl(float v, int lane) {
  v += dpp_or_zero<0x101, 0xf>(v);
  v += dpp_or_zero<0x102, 0xf>(v);
  v += dpp_or_zero<0x104, 0xf>(v);
  v += dpp_or_zero<0x108, 0xf>(v);
  const int vi = __builtin_bit_cast(int, v);
  const float t1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(vi, 16));
  const float t2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(vi, 32));
  const float t3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(vi, 48));
  const int row = lane >> 4;
  const float above = row == 0 ? (t1 + (t2 + t3)) : row == 1 ? (t2 + t3) : row == 2 ? t3 : 0.0f;
  return v + above;
}

// one loss sum of a 256-thread workgroup: the four waves' partial sums (lane 0 of wave wv holds v) through 16 B of LDS, one
// atomic per block
__device__ __forceinline__ void block_loss_add(float* part, int lane, int wv, float v, float scale, float* __restrict__ out) {
  if (lane == 0) part[wv] = v;
  __syncthreads();
  if (threadIdx.x == 0 && out) atomicAdd(out, (part[0] + part[1] + part[2] + part[3]) * scale);
}

// the workgroups of a flat launch (NERF_LAUNCH below): one lane per item, `block` lanes a workgroup
static inline unsigned blocks(int64_t n, int block) { return (unsigned)((n + block - 1) / block); }
}  // namespace nerf

#define NERF_REQUIRE(cond, code, ...) \
  do {                                \
    if (!(cond)) return nerf::fail(code, __VA_ARGS__); \
  } while (0)

// a check or a launch helper that returns a code: a failure returns it from the calling entry
#define NERF_TRY(call)             \
  do {                             \
    const int rc_ = (call);        \
    if (rc_) return rc_;           \
  } while (0)

// a HIP runtime call (a memset, a copy): a failure returns NERF_E_HIP with "<who>: <HIP's text>" from the calling entry
#define NERF_HIP(who, call)                                                                       \
  do {                                                                                            \
    const hipError_t e_ = (call);                                                                 \
    if (e_ != hipSuccess) return nerf::fail(NERF_E_HIP, "%s: %s", who, hipGetErrorString(e_));    \
  } while (0)

// Launches `kernel` with `blocks` workgroups of `threads` on hipStream_t `st`; a failed launch returns its code from the calling entry.
#define NERF_LAUNCH(what, kernel, blocks, threads, st, ...)                                        \
  do {                                                                                             \
    hipLaunchKernelGGL(kernel, dim3((unsigned)(blocks)), dim3(threads), 0, st, __VA_ARGS__);       \
    const int rc_ = nerf::check_launch(what);                                                      \
    if (rc_) return rc_;                                                                           \
  } while (0)
