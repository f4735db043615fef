// What the host side of every mesh unit carves its workspace with (simplify.hip, decimate.hip, smooth_ws.h, distance.hip, bvh_ws.h):
// the item limit, the workgroups over n items, and the bump carver.  A workspace is a run of regions, each rounded up to ALIGN
// bytes, in the order of the take() calls; with ws = NULL nothing is dereferenced and bytes() is the size the entry reports.
// Compiles without HIP (the *_ws_check.cpp programs of tests/ carve under a host compiler).
#pragma once
#include <stdint.h>

namespace nerf {
namespace {

constexpr int64_t MESH_MAX_ITEMS = 1 << 24;         // vertices, faces: 3 F corners fit an int

// the workgroups of `block` lanes over n items, as the int64_t the carves count in (common.h's blocks() is the launch's unsigned)
inline int64_t mesh_blocks(int64_t n, int block) { return (n + block - 1) / block; }

template <int ALIGN = 8>
struct WsCarver {
  uintptr_t p0, p;
  explicit WsCarver(void* ws) : p0(reinterpret_cast<uintptr_t>(ws)), p(p0) {}
  // the next region: `count` items of T, the cursor moved past them to the next multiple of ALIGN
  template <class T>
  T* take(int64_t count) {
    const uintptr_t at = p;
    p += (uintptr_t)((count * (int64_t)sizeof(T) + (ALIGN - 1)) & ~(int64_t)(ALIGN - 1));
    return reinterpret_cast<T*>(at);
  }
  int64_t bytes() const { return (int64_t)(p - p0); }
};

}  // namespace
}  // namespace nerf
