// The mip pyramid of the texture atlas of texture.h (mip.hip), the one statement in code of include/nerf_hip.h "texture mip
// pyramid".  Every float step rounds to float32 on its own (-ffp-contract=off); divisions are div_rn, square roots sqrt_rn.
//   levels   T_0 = T; T_{l+1} = (T_l + 1) / 2 (integers) while T_l > 2; at most NERF_MIP_MAX_LEVELS.  Level l is a whole atlas of the
//            same faces: tex_layout(F, T_l), the UVs of nerf_texture_uv(F, T_l).
//   reduce   fine (T, S = T + 2) -> coarse (T', S'), one lane per coarse atlas texel; tex_owner on the coarse layout gives the face
//            f and the local texel (i, j); a face >= F is black; only the fine image is read, never the mesh.
//            in-triangle, i + j <= T' - 1: x = (float)(i (T - 1)) / (float)(T' - 1), y likewise; r = (float)(T - 1) / (float)(T' - 1),
//            d = 0.25f r; c = tex_lookup(x, y); four antipodal tap pairs (x, y) +- o with o = (d, 0), (0, d), (d, d), (d, -d); a pair
//            counts only if both taps a lie in the closed triangle ax >= 0, ay >= 0, ax + ay <= (float)(T - 1) (the sum in
//            float32) and is then p = lookup(a) + lookup(b), else p = c + c; value = ((p0 + p1) + (p2 + p3)) 0.125f per channel;
//            byte = rintf(255 tex_unit(value)), the store of texture.hip.
//            gutter, the diagonals i + j = T' and then T' + 1, from the coarse bytes in integers: g(i, j) = v(i - 1, j) +
//            v(i, j - 1) - v(i - 1, j - 1) for i, j >= 1; g(i, 0) = 2 v(i - 1, 0) - v(i - 2, 0); g(0, j) = 2 v(0, j - 1) - v(0, j - 2);
//            clamped to [0, 255]; the second diagonal uses the clamped first.  A gutter lane recomputes the in-triangle bytes it
//            needs (at most seven), so one launch writes a level and the image depends on neither the chunk nor the launch shape.
//   lod      per face: raster_setup(cull = 0), the rasteriser's snapped face; not RASTER_OK: 0.  S = |D| (int64);
//            g = scale (sqrt_rn((float)S) / 256.0f), the leg in pixels of the right isosceles triangle of the face's screen area,
//            on which level l puts T_l - 1 texel steps.  One level or g >= T_0 - 1: 0; g <= T_{L-1} - 1: L - 1; else the l with
//            T_{l+1} - 1 <= g < T_l - 1 and lod = (float)l + ((float)(T_l - 1) - g) / (float)(T_l - T_{l+1}).
//   sample   lod clamped to [0, L - 1] (NaN -> 0); l = (int)floorf(lod), t = lod - (float)l; barycentrics clamped as the sampler of
//            texture.hip clamps them; c_l = tex_lookup on level l at (wb (T_l - 1), wc (T_l - 1)); t == 0: c_l, else
//            ((1.0f - t) c_l) + (t c_{l+1}); a face outside [0, F) reads black.
// The argument checks compile for the host; the device part is shared by the three kernels of mip.hip.
#pragma once
#include "texture.h"
#include "raster.h"

namespace nerf {
namespace {

constexpr int MIP_BLOCK = 256;
static_assert(NERF_MIP_MAX_LEVELS == 6, "64 -> 64, 32, 16, 8, 4, 2");

// the texels per leg of every level of a pyramid over T_0 = T (T >= 2): the count L, T_l into out[0 .. L)
__host__ __device__ __forceinline__ int mip_chain(int T, int* out) {
  int L = 0;
  out[L++] = T;
  while (T > 2 && L < NERF_MIP_MAX_LEVELS) {
    T = (T + 1) / 2;
    out[L++] = T;
  }
  return L;
}

// the levels of a launch of the sampler: passed to the kernel by value
struct MipLevels {
  const uint8_t* image[NERF_MIP_MAX_LEVELS];
  TexLayout lay[NERF_MIP_MAX_LEVELS];
  int L;
};

// the texel counts of a launch of the lod kernel
struct MipChain {
  int T[NERF_MIP_MAX_LEVELS];
  int L;
};

inline int mip_texels_check(const char* who, int T) {
  NERF_REQUIRE(T >= TEX_MIN_TEXELS && T <= TEX_MAX_TEXELS, NERF_E_SHAPE, "%s: need %d <= texels <= %d (got %d)", who, TEX_MIN_TEXELS,
               TEX_MAX_TEXELS, T);
  return NERF_OK;
}

// every argument of nerf_mip_reduce; fills both layouts.  *work: whether anything is to be launched
inline int mip_reduce_check(const char* who, const uint8_t* fine, int64_t F, int T, const uint8_t* coarse, int64_t p0, int64_t count,
                            TexLayout* lf, TexLayout* lc, bool* work) {
  *work = false;
  int rc = tex_layout(who, F, T, lf);
  if (rc) return rc;
  NERF_REQUIRE(T > 2, NERF_E_SHAPE, "%s: a level of %d texels a leg is the last one", who, T);
  rc = tex_layout(who, F, (T + 1) / 2, lc);
  if (!rc) rc = tex_chunk_check(who, *lc, p0, count);
  if (rc) return rc;
  if (count == 0) return NERF_OK;
  NERF_REQUIRE(fine && coarse, NERF_E_NULL, "%s: NULL pointer", who);
  *work = true;
  return NERF_OK;
}

// every argument of nerf_mip_lod; fills the chain
inline int mip_lod_check(const char* who, const float* verts, int64_t V, const int32_t* faces, int64_t F, const nerf_tsdf_view* view_host,
                         float near, int T, float scale, const float* lod, MipChain* chain, bool* work) {
  *work = false;
  int rc = mesh_check(who, V, F);
  if (!rc) rc = mip_texels_check(who, T);
  if (!rc) rc = camera_near_check(who, near);
  if (rc) return rc;
  NERF_REQUIRE(std::isfinite(scale) && scale > 0.0f, NERF_E_SHAPE, "%s: scale must be finite and > 0 (got %g)", who, (double)scale);
  rc = camera_view_check(who, view_host);
  if (rc) return rc;
  chain->L = mip_chain(T, chain->T);
  NERF_REQUIRE((lod && faces) || F == 0, NERF_E_NULL, "%s: NULL pointer", who);
  NERF_REQUIRE(verts || V == 0, NERF_E_NULL, "%s: NULL verts", who);
  *work = F > 0;
  return NERF_OK;
}

// every argument of nerf_mip_sample; fills the levels
inline int mip_sample_check(const char* who, const uint8_t* const* images_host, int64_t F, int T, const int32_t* face, const float* bary,
                            const float* lod, int per_face, int64_t n, const float* rgb, MipLevels* lv, bool* work) {
  *work = false;
  TexLayout top;
  const int rc = tex_layout(who, F, T, &top);
  if (rc) return rc;
  NERF_REQUIRE(per_face == 0 || per_face == 1, NERF_E_SHAPE, "%s: per_face must be 0 or 1 (got %d)", who, per_face);
  NERF_REQUIRE(n >= 0 && n <= ((int64_t)1 << 31) - 1, NERF_E_SHAPE, "%s: need 0 <= n < 2^31 (got %lld)", who, (long long)n);
  if (n == 0) return NERF_OK;
  NERF_REQUIRE(images_host && face && bary && lod && rgb, NERF_E_NULL, "%s: NULL pointer", who);
  int chain[NERF_MIP_MAX_LEVELS];
  lv->L = mip_chain(T, chain);
  for (int l = 0; l < NERF_MIP_MAX_LEVELS; ++l) {
    const int k = l < lv->L ? l : lv->L - 1;                  // (the unused slots repeat the last level: never read, never wild)
    NERF_REQUIRE(images_host[k], NERF_E_NULL, "%s: NULL image of level %d", who, k);
    lv->image[l] = images_host[k];
    const int rl = tex_layout(who, F, chain[k], &lv->lay[l]);
    if (rl) return rl;
  }
  *work = true;
  return NERF_OK;
}

#if defined(__HIPCC__)
// the byte of texture.hip's store
__device__ __forceinline__ int mip_byte(float v) { return (int)rintf(255.0f * tex_unit(v)); }
__device__ __forceinline__ int mip_clamp(int v) { return min(max(v, 0), 255); }

// the in-triangle texel (i, j), i + j <= T' - 1, of face f of the coarse level from the fine image: bytes into out[3]
__device__ __forceinline__ void mip_inner(const uint8_t* __restrict__ fine, const TexLayout& lf, int Tc, int f, int i, int j, int* out) {
  const float top = (float)(lf.T - 1), den = (float)(Tc - 1);
  const float x = div_rn((float)(i * (lf.T - 1)), den), y = div_rn((float)(j * (lf.T - 1)), den);
  const float d = 0.25f * div_rn(top, den);
  float c[3], sum[4][3];
  tex_lookup(fine, lf, f, x, y, c);
  const float ox[4] = {d, 0.0f, d, d}, oy[4] = {0.0f, d, d, 0.0f - d};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float ax = x + ox[k], ay = y + oy[k], bx = x - ox[k], by = y - oy[k];
    const bool both = ax >= 0.0f && ay >= 0.0f && ax + ay <= top && bx >= 0.0f && by >= 0.0f && bx + by <= top;
    if (both) {
      float a[3], b[3];
      tex_lookup(fine, lf, f, ax, ay, a);
      tex_lookup(fine, lf, f, bx, by, b);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) sum[k][ch] = a[ch] + b[ch];
    } else {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) sum[k][ch] = c[ch] + c[ch];
    }
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) out[ch] = mip_byte(((sum[0][ch] + sum[1][ch]) + (sum[2][ch] + sum[3][ch])) * 0.125f);
}

// a texel of the first gutter diagonal, i + j = T', from the three (two on a leg) in-triangle bytes beside it
__device__ __forceinline__ void mip_gutter1(const uint8_t* __restrict__ fine, const TexLayout& lf, int Tc, int f, int i, int j, int* out) {
  int a[3], b[3];
  if (i == 0 || j == 0) {
    const int di = j == 0 ? 1 : 0, dj = 1 - di;
    mip_inner(fine, lf, Tc, f, i - di, j - dj, a);
    mip_inner(fine, lf, Tc, f, i - 2 * di, j - 2 * dj, b);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) out[ch] = mip_clamp(2 * a[ch] - b[ch]);
    return;
  }
  int c[3];
  mip_inner(fine, lf, Tc, f, i - 1, j, a);
  mip_inner(fine, lf, Tc, f, i, j - 1, b);
  mip_inner(fine, lf, Tc, f, i - 1, j - 1, c);
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) out[ch] = mip_clamp(a[ch] + b[ch] - c[ch]);
}

// texel (i, j) of face f (inside [0, F)) of the coarse level, whichever kind it is
__device__ __forceinline__ void mip_texel(const uint8_t* __restrict__ fine, const TexLayout& lf, int Tc, int f, int i, int j, int* out) {
  const int s = i + j;
  if (s <= Tc - 1) return mip_inner(fine, lf, Tc, f, i, j, out);
  if (s == Tc) return mip_gutter1(fine, lf, Tc, f, i, j, out);
  int a[3], b[3];                                             // the second diagonal: i + j = T' + 1
  if (i == 0 || j == 0) {
    const int di = j == 0 ? 1 : 0, dj = 1 - di;
    mip_gutter1(fine, lf, Tc, f, i - di, j - dj, a);
    mip_inner(fine, lf, Tc, f, i - 2 * di, j - 2 * dj, b);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) out[ch] = mip_clamp(2 * a[ch] - b[ch]);
    return;
  }
  int c[3];
  mip_gutter1(fine, lf, Tc, f, i - 1, j, a);
  mip_gutter1(fine, lf, Tc, f, i, j - 1, b);
  mip_inner(fine, lf, Tc, f, i - 1, j - 1, c);
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) out[ch] = mip_clamp(a[ch] + b[ch] - c[ch]);
}

// the level of detail of a face whose snapped doubled screen area is S = |D| > 0
__device__ __forceinline__ float mip_lod(const MipChain& ch, int64_t S, float scale) {
  const float g = scale * div_rn(sqrt_rn((float)S), 256.0f);
  if (ch.L == 1 || g >= (float)(ch.T[0] - 1)) return 0.0f;
  float lod = (float)(ch.L - 1);                              // g <= T_{L-1} - 1 (and NaN, which the checks rule out)
#pragma unroll
  for (int l = 0; l + 1 < NERF_MIP_MAX_LEVELS; ++l) {
    if (l + 1 < ch.L && g < (float)(ch.T[l] - 1) && g >= (float)(ch.T[l + 1] - 1))
      lod = (float)l + div_rn((float)(ch.T[l] - 1) - g, (float)(ch.T[l] - ch.T[l + 1]));
  }
  return lod;
}
#endif

}  // namespace
}  // namespace nerf
