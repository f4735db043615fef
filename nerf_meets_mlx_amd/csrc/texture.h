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
// The layout helpers compile for host and device; the host checks use nerf::fail through NERF_REQUIRE.
#pragma once
#include "lattice.h"

namespace nerf {
namespace {

constexpr int TEX_BLOCK = 256;
constexpr int TEX_MIN_TEXELS = 2, TEX_MAX_TEXELS = 64;
constexpr int64_t TEX_MAX_FACES = 1 << 24;

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
  NERF_REQUIRE(F >= 0 && F <= TEX_MAX_FACES, NERF_E_SHAPE, "%s: need 0 <= F <= 2^24 (got %lld)", who, (long long)F);
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

}  // namespace
}  // namespace nerf
