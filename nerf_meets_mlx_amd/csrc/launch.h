// The launch of an MLP kernel (mlp*.hip): opt-in to dynamic LDS above 64 KiB, launch, check.  Grids that several units share.
#pragma once
#include "common.h"

namespace nerf {

// Dynamic LDS of a launch.  `optin` is what the kernel is opted in to when that is more than its own launch needs (mlp22.hip:
// every form gets the largest form's size).
struct Lds {
  int bytes, optin;
  Lds(int b) : bytes(b), optin(b) {}
  Lds(int b, int group_max) : bytes(b), optin(group_max) {}
};

// hipFuncSetAttribute applies to the current device: once per (kernel, device), DevOnce (common.h).  One flag per KERNEL, so
// kernels that are opted in together may name each other in either order and still meet one attribute call each.
template <auto K>
static void lds_optin(int dev, int bytes) {
  static DevOnce once;
  once.run(dev, [&] { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize, bytes); });
}

// Launches K and returns check_launch(what).  More than 64 KiB of dynamic LDS: K and the kernels WITH... are opted in first (a
// training step that was warmed up with one form of a kernel does not meet the other form's first opt-in later, inside a graph
// capture for instance).  64 KiB or less: no HIP call besides the launch.
template <auto K, auto... WITH, class... Args>
static int launch(const char* what, dim3 grid, dim3 block, Lds lds, hipStream_t s, const Args&... args) {
  if (lds.bytes > 64 * 1024) {
    const int dev = DevOnce::device();
    lds_optin<K>(dev, lds.optin);
    (lds_optin<WITH>(dev, lds.optin), ...);
  }
  hipLaunchKernelGGL(K, grid, block, lds.bytes, s, args...);
  return check_launch(what);
}

// grid of a persistent kernel: one workgroup per super-tile, at most `wgs`
static inline unsigned persistent_grid(int64_t nsuper, int64_t wgs) { return (unsigned)(nsuper < wgs ? nsuper : wgs); }
// grid of the 2 x 64 model's kernels: one workgroup per 8 tiles, at most 2048 (they stride over the rest)
static inline unsigned small_grid(int64_t ntiles) { return persistent_grid((ntiles + 7) / 8, 2048); }

// A runtime index 0 .. N-1 as a template argument: with_bool's sibling for three-way modes (fn receives std::integral_constant<int, I>).
template <int N, class Fn> static inline auto with_index(int i, Fn&& fn) {
  if constexpr (N > 1) { if (i < N - 1) return with_index<N - 1>(i, std::forward<Fn>(fn)); }
  return fn(std::integral_constant<int, N - 1>{});
}

}  // namespace nerf
