// A visibility-buffer rasteriser for finished meshes: which face a pixel of a posed pinhole camera sees, where on it, and how far.
// Semantics in include/nerf_hip.h "mesh rendering", stated in code in raster.h; tests/_raster_ref.py reproduces every output bit
// for bit.  No reference counterpart.  Coverage is exact int64 arithmetic on coordinates snapped to 1 / 256 pixel; visibility is one
// 64-bit atomicMin per covered pixel on the key (depth bits, face): a minimum does not depend on the order of its operands, so the
// buffer is bit-reproducible and independent of face order and launch shape.  No float atomics.
//   clear    one lane per pixel: the key all ones; the first four lanes zero the stats block.
//   draw     one lane per face does the setup (three gathered vertices, the projection, the drop tests) and the bounding box of
//            the snapped corners clipped to the image.  A face whose box has at most small_max pixels is walked by its own lane:
//            the 692 k faces of a marching-cubes mesh at 800^2 cover about a pixel each, and a wave per face would idle 63
//            lanes.  The others are taken one after another from the wave's __ballot mask: the owner's setup is broadcast with
//            __shfl and the 64 lanes walk the box in tiles of 8 x 8 pixels (eight keys of a row are 64 contiguous bytes), so a
//            face of hundreds of pixels does not serialise on one lane.  Both paths evaluate raster_pixel, so the keys do not
//            depend on small_max.  The atomics return nothing, so a lane issues them and goes on.  Reading the key with a plain
//            load first and skipping the atomic when the stored key is already <= this one (correct: keys only fall, so a stale
//            read can only cause an atomic that changes nothing) puts the load's latency in front of every covered pixel and
//            measured slower on all three meshes of DESIGN.md section 32; it is not shipped (-DRASTER_PREREAD=1 builds it).
//   resolve  one lane per pixel: the winner's setup and raster_pixel again -> face, (wb, wc), depth, acc.
//   shade    one lane per pixel: the barycentric sum of the vertex colours, or an rgb the caller looked up; background where empty.
#include "raster.h"

#ifndef RASTER_PREREAD
#define RASTER_PREREAD 0
#endif

namespace nerf {
namespace {

__device__ __forceinline__ void raster_put(unsigned long long* keys, int64_t p, unsigned long long key) {
#if RASTER_PREREAD
  if (keys[p] <= key) return;
#endif
  atomicMin(keys + p, key);
}

__global__ void __launch_bounds__(RASTER_BLOCK) raster_clear_kernel(unsigned long long* __restrict__ keys, int64_t n,
                                                                   unsigned long long* __restrict__ stats) {
  const int64_t p = (int64_t)blockIdx.x * RASTER_BLOCK + threadIdx.x;
  if (p < n) keys[p] = RASTER_EMPTY;
  if (p < 4) stats[p] = 0ull;
}

// ---- draw: per face 12 B of indices and 36 B of vertices gathered; per covered pixel one 8-byte atomic without a return
__global__ void __launch_bounds__(RASTER_BLOCK) raster_draw_kernel(const float* __restrict__ verts, int V, const int* __restrict__ faces,
                                                                  int F, int face_base, nerf_tsdf_view view, int H, int W, float near,
                                                                  int cull, int small_max, unsigned long long* keys,
                                                                  unsigned long long* __restrict__ stats) {
  const int f = blockIdx.x * RASTER_BLOCK + threadIdx.x;
  const int lane = threadIdx.x & (WAVE - 1);
  RasterFace rf = {};
  int why = -1, x0 = 0, x1 = -1, y0 = 0, y1 = -1;
  if (f < F) {
    why = raster_setup(verts, V, faces + 3 * (int64_t)f, view, near, cull, &rf);
    if (why == RASTER_OK) {
      const int xmin = min(rf.X[0], min(rf.X[1], rf.X[2])), xmax = max(rf.X[0], max(rf.X[1], rf.X[2]));
      const int ymin = min(rf.Y[0], min(rf.Y[1], rf.Y[2])), ymax = max(rf.Y[0], max(rf.Y[1], rf.Y[2]));
      x0 = max((xmin + (RASTER_SNAP - 1)) >> 8, 0);
      x1 = min(xmax >> 8, W - 1);
      y0 = max((ymin + (RASTER_SNAP - 1)) >> 8, 0);
      y1 = min(ymax >> 8, H - 1);
    }
  }
  const bool live = why == RASTER_OK && x0 <= x1 && y0 <= y1;
  const bool own = live && (x1 - x0 + 1) * (y1 - y0 + 1) <= small_max;         // (at most 2^28 pixels: an int)
  unsigned long long updates = 0ull;
  float wb, wc, z;
  if (own) {
    const int id = face_base + f;
    for (int py = y0; py <= y1; ++py)
      for (int px = x0; px <= x1; ++px)
        if (raster_pixel(rf, px, py, &wb, &wc, &z)) {
          raster_put(keys, (int64_t)py * W + px, raster_key(z, id));
          ++updates;
        }
  }
  unsigned long long big = __ballot(live && !own);
  while (big) {                                                                // (uniform over the wave)
    const int src = __ffsll((long long)big) - 1;
    big &= big - 1ull;
    RasterFace bf;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      bf.X[c] = __shfl(rf.X[c], src, WAVE);
      bf.Y[c] = __shfl(rf.Y[c], src, WAVE);
      bf.z[c] = __shfl(rf.z[c], src, WAVE);
    }
    bf.s = __shfl(rf.s, src, WAVE);
    const int bx0 = __shfl(x0, src, WAVE), bx1 = __shfl(x1, src, WAVE), by0 = __shfl(y0, src, WAVE), by1 = __shfl(y1, src, WAVE);
    const int id = face_base + __shfl(f, src, WAVE);
    for (int ty = by0; ty <= by1; ty += 8)
      for (int tx = bx0; tx <= bx1; tx += 8) {
        const int px = tx + (lane & 7), py = ty + (lane >> 3);
        if (px <= bx1 && py <= by1 && raster_pixel(bf, px, py, &wb, &wc, &z)) {
          raster_put(keys, (int64_t)py * W + px, raster_key(z, id));
          ++updates;
        }
      }
  }
  // the wave's counts: three popcounts and one sum, then at most four atomics from lane 0 (integer sums: order-independent)
  const unsigned long long drawn = __popcll(__ballot(why == RASTER_OK));
  const unsigned long long depth = __popcll(__ballot(why == RASTER_DROP_DEPTH));
  const unsigned long long other = __popcll(__ballot(why == RASTER_DROP_OTHER));
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) updates += __shfl_xor(updates, o, WAVE);
  if (lane == 0) {
    if (drawn) atomicAdd(stats + 0, drawn);
    if (depth) atomicAdd(stats + 1, depth);
    if (other) atomicAdd(stats + 2, other);
    if (updates) atomicAdd(stats + 3, updates);
  }
}

// ---- resolve: 8 B read per pixel, the winner's 48 B gathered, 20 B written
__global__ void __launch_bounds__(RASTER_BLOCK) raster_resolve_kernel(const unsigned long long* __restrict__ keys,
                                                                     const float* __restrict__ verts, int V,
                                                                     const int* __restrict__ faces, int F, nerf_tsdf_view view, int H, int W,
                                                                     float near, int* __restrict__ face, float* __restrict__ bary,
                                                                     float* __restrict__ depth, float* __restrict__ acc) {
  const int64_t p = (int64_t)blockIdx.x * RASTER_BLOCK + threadIdx.x;
  if (p >= (int64_t)H * W) return;
  const unsigned long long key = keys[p];
  const unsigned id = (unsigned)key;
  int out_face = -1;
  float wb = 0.0f, wc = 0.0f, z = 0.0f, a = 0.0f;
  RasterFace rf;
  if (key != RASTER_EMPTY && id < (unsigned)F && raster_setup(verts, V, faces + 3 * (int64_t)id, view, near, 0, &rf) == RASTER_OK) {
    const int py = (int)(p / W), px = (int)(p - (int64_t)py * W);
    float b, c, d;
    if (raster_pixel(rf, px, py, &b, &c, &d)) {
      out_face = (int)id; wb = b; wc = c; z = d; a = 1.0f;
    }
  }
  face[p] = out_face;
  bary[2 * p] = wb;
  bary[2 * p + 1] = wc;
  depth[p] = z;
  acc[p] = a;
}

// ---- shade: 12 B read per pixel and three gathered colours (or 12 B of rgb_in), 12 B written
__global__ void __launch_bounds__(RASTER_BLOCK) raster_shade_kernel(const int* __restrict__ face, const float* __restrict__ bary,
                                                                   const int* __restrict__ faces, int V, int F,
                                                                   const float* __restrict__ colors, const float* __restrict__ rgb_in,
                                                                   const float* __restrict__ background, int per_pixel, int64_t n,
                                                                   float* __restrict__ rgb) {
  const int64_t p = (int64_t)blockIdx.x * RASTER_BLOCK + threadIdx.x;
  if (p >= n) return;
  const int f = face[p];
  const float* bg = background + (per_pixel ? 3 * p : 0);
  float out[3] = {bg[0], bg[1], bg[2]};
  if (f >= 0) {
    if (rgb_in) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) out[ch] = rgb_in[3 * p + ch];
    } else if (f < F) {
      int g[3];
      if (mesh_corners(faces + 3 * (int64_t)f, V, g)) {
        const float wb = bary[2 * p], wc = bary[2 * p + 1];
        const float wa = (1.0f - wb) - wc;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) out[ch] = (wa * colors[3 * g[0] + ch] + wb * colors[3 * g[1] + ch]) + wc * colors[3 * g[2] + ch];
      }
    }
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) rgb[3 * p + ch] = out[ch];
}

}  // namespace
}  // namespace nerf

using namespace nerf;

extern "C" int nerf_raster_clear(uint64_t* keys, int H, int W, uint64_t* stats, void* stream) {
  const int rc = camera_image_check("nerf_raster_clear", H, W, CAMERA_MAX_SIDE);
  if (rc) return rc;
  NERF_REQUIRE(keys && stats, NERF_E_NULL, "nerf_raster_clear: NULL pointer");
  const int64_t n = (int64_t)H * W;
  NERF_LAUNCH("nerf_raster_clear", raster_clear_kernel, blocks(n, RASTER_BLOCK), RASTER_BLOCK, as_stream(stream),
              reinterpret_cast<unsigned long long*>(keys), n, reinterpret_cast<unsigned long long*>(stats));
  return NERF_OK;
}

extern "C" int nerf_raster_draw(const float* verts, int64_t V, const int32_t* faces, int64_t F, int64_t face_base,
                                const nerf_tsdf_view* view_host, int H, int W, float near, int cull_backfaces, int small_max,
                                uint64_t* keys, uint64_t* stats, void* stream) {
  const char* who = "nerf_raster_draw";
  int rc = camera_image_check(who, H, W, CAMERA_MAX_SIDE);
  if (!rc) rc = mesh_check(who, V, F);
  if (rc) return rc;
  NERF_REQUIRE(face_base >= 0 && face_base <= MESH_MAX_ITEMS - F, NERF_E_SHAPE, "%s: need 0 <= face_base <= 2^24 - F (got %lld)", who,
               (long long)face_base);
  NERF_REQUIRE(cull_backfaces == 0 || cull_backfaces == 1, NERF_E_SHAPE, "%s: cull_backfaces must be 0 or 1 (got %d)", who, cull_backfaces);
  NERF_REQUIRE(small_max >= 0 && small_max <= RASTER_MAX_SMALL, NERF_E_SHAPE, "%s: need 0 <= small_max <= 2^30 (got %d)", who, small_max);
  rc = camera_near_check(who, near);
  if (!rc) rc = camera_view_check(who, view_host);
  if (rc) return rc;
  NERF_REQUIRE(keys && stats && (faces || F == 0) && (verts || V == 0), NERF_E_NULL, "%s: NULL pointer", who);
  if (F == 0) return NERF_OK;
  NERF_LAUNCH(who, raster_draw_kernel, blocks(F, RASTER_BLOCK), RASTER_BLOCK, as_stream(stream), verts, (int)V, faces, (int)F, (int)face_base,
              *view_host, H, W, near, cull_backfaces, small_max, reinterpret_cast<unsigned long long*>(keys),
              reinterpret_cast<unsigned long long*>(stats));
  return NERF_OK;
}

extern "C" int nerf_raster_resolve(const uint64_t* keys, const float* verts, int64_t V, const int32_t* faces, int64_t F,
                                   const nerf_tsdf_view* view_host, int H, int W, float near, int32_t* face, float* bary, float* depth,
                                   float* acc, void* stream) {
  const char* who = "nerf_raster_resolve";
  int rc = camera_image_check(who, H, W, CAMERA_MAX_SIDE);
  if (!rc) rc = mesh_check(who, V, F);
  if (!rc) rc = camera_near_check(who, near);
  if (!rc) rc = camera_view_check(who, view_host);
  if (rc) return rc;
  NERF_REQUIRE(keys && face && bary && depth && acc && (faces || F == 0) && (verts || V == 0), NERF_E_NULL, "%s: NULL pointer", who);
  NERF_LAUNCH(who, raster_resolve_kernel, blocks((int64_t)H * W, RASTER_BLOCK), RASTER_BLOCK, as_stream(stream),
              reinterpret_cast<const unsigned long long*>(keys), verts, (int)V, faces, (int)F, *view_host, H, W, near, face, bary, depth, acc);
  return NERF_OK;
}

extern "C" int nerf_raster_shade(const int32_t* face, const float* bary, const int32_t* faces, int64_t V, int64_t F, const float* colors,
                                 const float* rgb_in, const float* background, int per_pixel, int H, int W, float* rgb, void* stream) {
  const char* who = "nerf_raster_shade";
  int rc = camera_image_check(who, H, W, CAMERA_MAX_SIDE);
  if (!rc) rc = mesh_check(who, V, F);
  if (rc) return rc;
  NERF_REQUIRE(per_pixel == 0 || per_pixel == 1, NERF_E_SHAPE, "%s: per_pixel must be 0 or 1 (got %d)", who, per_pixel);
  NERF_REQUIRE((colors != nullptr) != (rgb_in != nullptr), NERF_E_NULL, "%s: need exactly one of colors and rgb_in", who);
  NERF_REQUIRE(face && background && rgb && (rgb_in || (bary && (faces || F == 0))), NERF_E_NULL, "%s: NULL pointer", who);
  const int64_t n = (int64_t)H * W;
  NERF_LAUNCH(who, raster_shade_kernel, blocks(n, RASTER_BLOCK), RASTER_BLOCK, as_stream(stream), face, bary, faces, (int)V, (int)F, colors,
              rgb_in, background, per_pixel, n, rgb);
  return NERF_OK;
}
