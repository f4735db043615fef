// The visibility-buffer rasteriser of a triangle mesh (raster.hip), the one statement in code of include/nerf_hip.h "mesh rendering":
//   camera   camera.h: camera_point, then camera_pixel, on every vertex; the tests follow the division; depth is zc
//   snap     X = (int)rintf(u * 256), Y = (int)rintf(v * 256): screen coordinates in 1 / 256 pixel
//   guard    |u|, |v| <= 2^20 pixels, tested on the floats before the cast, so |X|, |Y| <= 2^28: a difference of two coordinates is
//            below 2^30 (an int), a product of two differences below 2^59 and a difference of two products below 2^60 (an int64)
//   drop     index outside [0, V) or a non-finite vertex: other; else a vertex with !(near <= zc < inf) or outside the guard band:
//            depth; else doubled area 0, or facing away with cull: other.  Never clipped.
//   area     D = (Xb - Xa)(Yc - Ya) - (Yb - Ya)(Xc - Xa); y points down on the screen, so a face that is counter-clockwise seen from
//            the camera (a front face of the project's meshes) has D < 0.  s = sign(D), S = s D > 0.
//   cover    E(U, V; P) = (Vx - Ux)(Py - Uy) - (Vy - Uy)(Px - Ux) at P = (256 px, 256 py); Ea = s E(B, C; P), Eb = s E(C, A; P),
//            Ec = s E(A, B; P); Ea + Eb + Ec = S exactly; covered iff all three >= 0
//   pixel    qa = (float)Ea / za, qb, qc likewise; Q = (qa + qb) + qc; wb = qb / Q; wc = qc / Q; z = (float)S / Q
//   key      ((uint64)float_bits(z) << 32) | (uint32)face, minimised; all ones = empty
// Everything below is device code shared by the draw and the resolve, which therefore compute the same bits.
#pragma once
#include "camera.h"

namespace nerf {
namespace {

constexpr int RASTER_BLOCK = 256;
constexpr int RASTER_MAX_SMALL = 1 << 30;
constexpr int RASTER_SNAP = 256;                               // sub-pixel steps
constexpr float RASTER_GUARD = 1048576.0f;                     // 2^20 pixels
constexpr unsigned long long RASTER_EMPTY = ~0ull;
constexpr int RASTER_OK = 0, RASTER_DROP_DEPTH = 1, RASTER_DROP_OTHER = 2;

#if defined(__HIPCC__)
// a face on the screen: snapped corners, camera depths, orientation
struct RasterFace {
  int X[3], Y[3];
  float z[3];
  int s;                                                       // sign of D
};

__device__ __forceinline__ int64_t raster_edge(int Ux, int Uy, int Vx, int Vy, int Px, int Py) {
  return (int64_t)(Vx - Ux) * (int64_t)(Py - Uy) - (int64_t)(Vy - Uy) * (int64_t)(Px - Ux);
}

// RASTER_OK and the face, or why it is dropped; nothing is read through an index outside [0, V)
__device__ __forceinline__ int raster_setup(const float* __restrict__ verts, int V, const int* __restrict__ idx, const nerf_tsdf_view& vw,
                                            float near, int cull, RasterFace* out) {
  int g[3];
  if (!mesh_corners(idx, V, g)) return RASTER_DROP_OTHER;
  float u[3], v[3];
  bool finite = true, seen = true;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float p[3] = {verts[3 * g[c]], verts[3 * g[c] + 1], verts[3 * g[c] + 2]};
    finite = finite && fabsf(p[0]) <= 3.402823466e+38f && fabsf(p[1]) <= 3.402823466e+38f && fabsf(p[2]) <= 3.402823466e+38f;
    float cam[3];
    camera_point(vw, p, cam);
    out->z[c] = cam[2];
    camera_pixel(vw, cam, &u[c], &v[c]);
    seen = seen && cam[2] >= near && cam[2] <= 3.402823466e+38f;
  }
  if (!finite) return RASTER_DROP_OTHER;
  if (!seen) return RASTER_DROP_DEPTH;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (!(fabsf(u[c]) <= RASTER_GUARD && fabsf(v[c]) <= RASTER_GUARD)) return RASTER_DROP_DEPTH;        // (NaN fails here)
    out->X[c] = (int)rintf(u[c] * (float)RASTER_SNAP);
    out->Y[c] = (int)rintf(v[c] * (float)RASTER_SNAP);
  }
  const int64_t D = raster_edge(out->X[0], out->Y[0], out->X[1], out->Y[1], out->X[2], out->Y[2]);
  if (D == 0 || (cull && D > 0)) return RASTER_DROP_OTHER;
  out->s = D > 0 ? 1 : -1;
  return RASTER_OK;
}

// whether the centre of pixel (px, py) is covered, and there (wb, wc, z)
__device__ __forceinline__ bool raster_pixel(const RasterFace& f, int px, int py, float* wb, float* wc, float* z) {
  const int Px = RASTER_SNAP * px, Py = RASTER_SNAP * py;
  const int64_t Ea = f.s * raster_edge(f.X[1], f.Y[1], f.X[2], f.Y[2], Px, Py);
  const int64_t Eb = f.s * raster_edge(f.X[2], f.Y[2], f.X[0], f.Y[0], Px, Py);
  const int64_t Ec = f.s * raster_edge(f.X[0], f.Y[0], f.X[1], f.Y[1], Px, Py);
  if ((Ea | Eb | Ec) < 0) return false;
  const float qa = div_rn((float)Ea, f.z[0]), qb = div_rn((float)Eb, f.z[1]), qc = div_rn((float)Ec, f.z[2]);
  const float Q = (qa + qb) + qc;
  *wb = div_rn(qb, Q);
  *wc = div_rn(qc, Q);
  *z = div_rn((float)((Ea + Eb) + Ec), Q);
  return true;
}

__device__ __forceinline__ unsigned long long raster_key(float z, int face) {
  return ((unsigned long long)(unsigned)__float_as_int(z) << 32) | (unsigned long long)(unsigned)face;
}
#endif

}  // namespace
}  // namespace nerf
