// The texture atlas of a triangle mesh (texture.hip), the one statement in code of include/nerf_hip.h "texture atlas":
//   cell     two faces share a square of S = T + 2 texels a side; face 2c owns the texels (i, j) of cell c with i + j <= S - 1, face
//            2c + 1 the others, seen mirrored: (i, j) -> (S - 1 - i, S - 1 - j)
//   atlas    C = ceil(sqrt(ceil(F / 2))) >= 1 cells per row, W = C S, H = max(1, ceil(cells / C)) S, row 0 on top, raster index
//            p = X + W Y (int64); texel (X, Y) lies in cell (Y / S) C + X / S at (X mod S, Y mod S)
//   corners  a, b, c at the centres of the local texels (0, 0), (T - 1, 0), (0, T - 1): texel (i, j) has the barycentrics
//            wb = i / (T - 1), wc = j / (T - 1), wa = (1 - wb) - wc, not clamped: the gutter along the hypotenuse is extrapolated
//   lookup   bilinear, corner (i0, j0) = the floors clamped to [0, S - 2], fractions (fx, fy) = x - i0, y - j0;
//            ((w00 c00 + w10 c10) + w01 c01) + w11 c11 with w00 = (1 - fx)(1 - fy), w10 = fx (1 - fy), w01 = (1 - fx) fy,
//            w11 = fx fy and c = (float)byte / 255.0f, every operation rounded to float32 on its own
// The layout helpers compile for host and device; the host checks use nerf::fail through NERF_REQUIRE.  The device part below them
// (a texel's face, barycentrics, position and normal) is shared by texture.hip and project.hip, which therefore see the same texel;
// the bilinear lookup is shared by texture.hip and mip.hip, which therefore read the same colour.
#pragma once
#include "lattice.h"

namespace nerf {
namespace {

constexpr int TEX_BLOCK = 256;
constexpr int TEX_MIN_TEXELS = 2, TEX_MAX_TEXELS = 64;

struct TexLayout {
  int W, H, C, S, T;
  int F;
};

// the smallest C >= 1 with C C >= cells
inline int tex_cells_per_row(int64_t cells) {
  int64_t c = (int64_t)std::sqrt((double)cells);
  while (c * c < cells) ++c;
  while (c > 1 && (c - 1) * (c - 1) >= cells) --c;
  return (int)(c < 1 ? 1 : c);
}

// W, H, C, S of F faces at T texels per leg; NERF_E_SHAPE with the largest T that fits when a side exceeds NERF_TEXTURE_MAX_SIDE
inline int tex_layout(const char* who, int64_t F, int T, TexLayout* lay) {
  const int rc = mesh_check(who, 0, F);
  if (rc) return rc;
  NERF_REQUIRE(T >= TEX_MIN_TEXELS && T <= TEX_MAX_TEXELS, NERF_E_SHAPE, "%s: need %d <= texels <= %d (got %d)", who, TEX_MIN_TEXELS,
               TEX_MAX_TEXELS, T);
  const int64_t cells = (F + 1) / 2;
  const int C = tex_cells_per_row(cells), S = T + 2;
  const int64_t rows = (cells + C - 1) / C;
  const int64_t W = (int64_t)C * S, H = (rows < 1 ? 1 : rows) * S;
  NERF_REQUIRE(W <= NERF_TEXTURE_MAX_SIDE && H <= NERF_TEXTURE_MAX_SIDE, NERF_E_SHAPE,
               "%s: an atlas of %lld x %lld texels for %lld faces at texels = %d exceeds %d a side; the largest texels that fits is %d%s",
               who, (long long)W, (long long)H, (long long)F, T, NERF_TEXTURE_MAX_SIDE, NERF_TEXTURE_MAX_SIDE / C - 2,
               NERF_TEXTURE_MAX_SIDE / C - 2 < TEX_MIN_TEXELS ? " (none)" : "");
  *lay = TexLayout{(int)W, (int)H, C, S, T, (int)F};
  return NERF_OK;
}

// the mesh arguments of rows, store and sample, and the chunk [p0, p0 + count) of the atlas that rows, store and project.hip walk
inline int tex_mesh_check(const char* who, int64_t V, int64_t F, int T, TexLayout* lay) {
  const int rc = mesh_check(who, V, F);
  return rc ? rc : tex_layout(who, F, T, lay);
}
inline int tex_chunk_check(const char* who, const TexLayout& lay, int64_t p0, int64_t count) {
  const int64_t P = (int64_t)lay.W * lay.H;
  NERF_REQUIRE(p0 >= 0 && count >= 0 && p0 <= P && count <= P - p0, NERF_E_SHAPE,
               "%s: the chunk [%lld, %lld + %lld) leaves the atlas of %lld texels", who, (long long)p0, (long long)p0, (long long)count,
               (long long)P);
  return NERF_OK;
}

// the face of atlas texel (X, Y) and its local texel (i, j), mirrored for the odd face; a face >= F is unused
__host__ __device__ __forceinline__ int tex_owner(const TexLayout& l, int X, int Y, int* i, int* j) {
  const int c = (Y / l.S) * l.C + X / l.S;
  int a = X % l.S, b = Y % l.S;
  const bool odd = a + b > l.S - 1;
  if (odd) { a = l.S - 1 - a; b = l.S - 1 - b; }
  *i = a;
  *j = b;
  return 2 * c + (odd ? 1 : 0);
}

// the atlas texel of local texel (i, j) of face f
__host__ __device__ __forceinline__ void tex_place(const TexLayout& l, int f, int i, int j, int* X, int* Y) {
  const int c = f >> 1;
  if (f & 1) { i = l.S - 1 - i; j = l.S - 1 - j; }
  *X = (c % l.C) * l.S + i;
  *Y = (c / l.C) * l.S + j;
}

#if defined(__HIPCC__)
__device__ __forceinline__ float tex_pos(float x) { return x > 0.0f ? x : 0.0f; }                 // NaN -> 0
__device__ __forceinline__ float tex_unit(float x) { x = tex_pos(x); return x < 1.0f ? x : 1.0f; }

// the corners of face f; false for an unused face (f outside [0, F)) or one with an index outside [0, V): nothing is read through it
__device__ __forceinline__ bool tex_face(const int* __restrict__ faces, int f, int F, int V, int* g) {
  return f >= 0 && f < F && mesh_corners(faces + 3 * (int64_t)f, V, g);
}

// position x and unit normal n (0 where the interpolated normal has no direction) of the point with barycentrics (wb, wc) of the
// face with corners g: the texel of the rows kernel, the sample of the sampler and the texel the projective bake observes
__device__ __forceinline__ void tex_point(const float* __restrict__ verts, const float* __restrict__ normals, const int* g, float wb,
                                          float wc, float* x, float* n) {
  const float wa = (1.0f - wb) - wc;
  const float pa = tex_pos(wa), pb = tex_pos(wb), pc = tex_pos(wc);
  float m[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    x[a] = (wa * verts[3 * g[0] + a] + wb * verts[3 * g[1] + a]) + wc * verts[3 * g[2] + a];
    m[a] = (pa * normals[3 * g[0] + a] + pb * normals[3 * g[1] + a]) + pc * normals[3 * g[2] + a];
  }
  const float len = sqrt_rn((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
  const bool ok = len > 0.0f && len <= 3.402823466e+38f;
#pragma unroll
  for (int a = 0; a < 3; ++a) n[a] = ok ? div_rn(m[a], len) : 0.0f;
}

// texel p of the atlas: its face's corners g and its barycentrics; false for a texel of no face or of a face with a bad index
__device__ __forceinline__ bool tex_texel(const TexLayout& lay, const int* __restrict__ faces, int V, int64_t p, int* g, float* wb,
                                          float* wc) {
  const int Y = (int)(p / lay.W), X = (int)(p - (int64_t)Y * lay.W);
  int i, j;
  const int f = tex_owner(lay, X, Y, &i, &j);
  if (!tex_face(faces, f, lay.F, V, g)) return false;
  const float d = (float)(lay.T - 1);
  *wb = div_rn((float)i, d);
  *wc = div_rn((float)j, d);
  return true;
}

// the bilinear `lookup` of the header at the local texel coordinates (x, y) of face f (inside [0, F)): rgb into out[3].  The one
// copy: tex_sample_kernel calls it at (wb (T - 1), wc (T - 1)), mip.hip at its taps and on every level of a pyramid.
__device__ __forceinline__ void tex_lookup(const uint8_t* __restrict__ image, const TexLayout& lay, int f, float x, float y, float* out) {
  const int i0 = min(max((int)floorf(x), 0), lay.S - 2), j0 = min(max((int)floorf(y), 0), lay.S - 2);
  const float fx = x - (float)i0, fy = y - (float)j0;
  const float gx = 1.0f - fx, gy = 1.0f - fy;
  const float w[4] = {gx * gy, fx * gy, gx * fy, fx * fy};
  const uint8_t* t[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int X, Y;
    tex_place(lay, f, i0 + (k & 1), j0 + (k >> 1), &X, &Y);
    t[k] = image + 3 * ((int64_t)Y * lay.W + X);
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    float c[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = div_rn((float)t[k][ch], 255.0f);
    out[ch] = ((w[0] * c[0] + w[1] * c[1]) + w[2] * c[2]) + w[3] * c[3];
  }
}
#endif

}  // namespace
}  // namespace nerf
