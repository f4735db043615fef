// Texture atlas of a finished mesh: one right triangle of T texels a leg per face, two faces to a cell (texture.h), baked by one
// field query per texel.  Semantics in include/nerf_hip.h "texture atlas"; tests/_texture_ref.py reproduces every output bit for
// bit.  No reference counterpart.  No atomics, no host read, no workspace: every output element has one writer.
//   rows     one lane per texel of a chunk of the atlas in raster order: face, barycentrics, position, direction -> the colour row
//            [x, -n, 0, 0, -n] of the vertex colour query.  A workgroup's 256 rows go through 11 KiB of LDS (stride 11 words: no
//            bank conflict) and leave as 11 fully coalesced word stores per lane instead of 11 stores 44 bytes apart.
//   store    one lane per texel: one 16-byte load of raw, three byte stores.  Packing four texels a lane into one 12-byte store
//            measured slower and is not shipped.
//   uv       one lane per face, 24 bytes.
//   sample   one lane per surface sample: a bilinear lookup in the face's own texels (tex_lookup of texture.h, which mip.hip
//            shares), and optionally the query row of the very point, by the device function of the rows kernel.
#include "texture.h"

namespace nerf {
namespace {

// row `id` of `rows` (LDS or global): the point with barycentrics (wb, wc) of the face with corners g, looking along -normal
__device__ __forceinline__ void tex_write_row(float* rows, int id, const float* __restrict__ verts, const float* __restrict__ normals,
                                              const int* g, float wb, float wc) {
  float x[3], n[3];
  tex_point(verts, normals, g, wb, wc, x, n);
  write_color_row(rows, id, x, n);
}

__device__ __forceinline__ void tex_zero_row(float* rows, int id) {
#pragma unroll
  for (int k = 0; k < NERF_RAY_STRIDE; ++k) rows[id * NERF_RAY_STRIDE + k] = 0.0f;
}

// the workgroup's staged rows -> rows [first, first + live) of the output, consecutive lanes writing consecutive words
__device__ __forceinline__ void tex_flush_rows(const float* stage, float* __restrict__ out, int64_t first, int live) {
  __syncthreads();
  float* dst = out + first * NERF_RAY_STRIDE;
  for (int k = threadIdx.x; k < live * NERF_RAY_STRIDE; k += TEX_BLOCK) dst[k] = stage[k];
}

// ---- rows: per texel 12 B of face indices and 72 B of corners gathered (cache hits: a face has S^2 / 2 texels), 44 B written
__global__ void __launch_bounds__(TEX_BLOCK) tex_rows_kernel(const float* __restrict__ verts, const float* __restrict__ normals, int V,
                                                            const int* __restrict__ faces, TexLayout lay, int64_t p0, int64_t count,
                                                            float* __restrict__ rows) {
  __shared__ float stage[TEX_BLOCK * NERF_RAY_STRIDE];
  const int64_t first = (int64_t)blockIdx.x * TEX_BLOCK, q = first + threadIdx.x;
  if (q < count) {
    const int64_t p = p0 + q;
    int g[3];
    float wb, wc;
    if (tex_texel(lay, faces, V, p, g, &wb, &wc)) tex_write_row(stage, threadIdx.x, verts, normals, g, wb, wc);
    else tex_zero_row(stage, threadIdx.x);
  }
  const int64_t left = count - first;
  tex_flush_rows(stage, rows, first, (int)(left < TEX_BLOCK ? left : TEX_BLOCK));
}

// ---- store: per texel 16 B read in one load and 3 B written; a wave's 192 bytes are contiguous
__global__ void __launch_bounds__(TEX_BLOCK) tex_store_kernel(const float4* __restrict__ raw, int V, const int* __restrict__ faces,
                                                             TexLayout lay, int64_t p0, int64_t count, uint8_t* __restrict__ image) {
  const int64_t q = (int64_t)blockIdx.x * TEX_BLOCK + threadIdx.x;
  if (q >= count) return;
  const int64_t p = p0 + q;
  const int Y = (int)(p / lay.W), X = (int)(p - (int64_t)Y * lay.W);
  int i, j, g[3];
  const int f = tex_owner(lay, X, Y, &i, &j);
  uint8_t b[3] = {0, 0, 0};
  if (tex_face(faces, f, lay.F, V, g)) {
    const float4 c = raw[q];
    b[0] = (uint8_t)rintf(255.0f * tex_unit(c.x));
    b[1] = (uint8_t)rintf(255.0f * tex_unit(c.y));
    b[2] = (uint8_t)rintf(255.0f * tex_unit(c.z));
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) image[3 * p + ch] = b[ch];
}

// ---- uv: the three corners of a face at the centres of their texels, v upwards (OBJ)
__global__ void __launch_bounds__(TEX_BLOCK) tex_uv_kernel(TexLayout lay, float* __restrict__ uv) {
  const int f = blockIdx.x * TEX_BLOCK + threadIdx.x;
  if (f >= lay.F) return;
  const int ci[3] = {0, lay.T - 1, 0}, cj[3] = {0, 0, lay.T - 1};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    int X, Y;
    tex_place(lay, f, ci[c], cj[c], &X, &Y);
    uv[6 * (int64_t)f + 2 * c] = div_rn((float)X + 0.5f, (float)lay.W);
    uv[6 * (int64_t)f + 2 * c + 1] = 1.0f - div_rn((float)Y + 0.5f, (float)lay.H);
  }
}

// ---- sample: 12 B read per sample, twelve gathered bytes of the image, 12 B (and 44 B) written
__global__ void __launch_bounds__(TEX_BLOCK) tex_sample_kernel(const uint8_t* __restrict__ image, const float* __restrict__ verts,
                                                              const float* __restrict__ normals, int V, const int* __restrict__ faces,
                                                              TexLayout lay, const int* __restrict__ sface, const float* __restrict__ bary,
                                                              int64_t n, float* __restrict__ rgb, float* __restrict__ rows) {
  __shared__ float stage[TEX_BLOCK * NERF_RAY_STRIDE];
  const int64_t first = (int64_t)blockIdx.x * TEX_BLOCK, s = first + threadIdx.x;
  if (s < n) {
    const int f = sface[s];
    const float wb = tex_unit(bary[2 * s]);
    const float hi = 1.0f - wb;
    float wc = tex_pos(bary[2 * s + 1]);
    wc = wc < hi ? wc : hi;
    float out[3] = {0.0f, 0.0f, 0.0f};
    if (f >= 0 && f < lay.F) {
      const float d = (float)(lay.T - 1);
      tex_lookup(image, lay, f, wb * d, wc * d, out);
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) rgb[3 * s + ch] = out[ch];
    if (rows) {
      int g[3];
      if (tex_face(faces, f, lay.F, V, g)) tex_write_row(stage, threadIdx.x, verts, normals, g, wb, wc);
      else tex_zero_row(stage, threadIdx.x);
    }
  }
  if (rows) {                                                  // (uniform: every lane of the workgroup takes the barrier)
    const int64_t left = n - first;
    tex_flush_rows(stage, rows, first, (int)(left < TEX_BLOCK ? left : TEX_BLOCK));
  }
}

}  // namespace
}  // namespace nerf

using namespace nerf;

extern "C" int nerf_texture_layout(int64_t F, int texels, int64_t* out) {
  TexLayout lay;
  const int rc = tex_layout("nerf_texture_layout", F, texels, &lay);
  if (rc) return rc;
  NERF_REQUIRE(out, NERF_E_NULL, "nerf_texture_layout: NULL out");
  out[0] = lay.W; out[1] = lay.H; out[2] = lay.C; out[3] = lay.S;
  return NERF_OK;
}

extern "C" int nerf_texture_rows(const float* verts, const float* normals, int64_t V, const int32_t* faces, int64_t F, int texels,
                                 int64_t p0, int64_t count, float* rows, void* stream) {
  TexLayout lay;
  int rc = tex_mesh_check("nerf_texture_rows", V, F, texels, &lay);
  if (!rc) rc = tex_chunk_check("nerf_texture_rows", lay, p0, count);
  if (rc) return rc;
  if (count == 0) return NERF_OK;
  NERF_REQUIRE(rows && (faces || F == 0) && ((verts && normals) || V == 0), NERF_E_NULL, "nerf_texture_rows: NULL pointer");
  NERF_LAUNCH("nerf_texture_rows", tex_rows_kernel, blocks(count, TEX_BLOCK), TEX_BLOCK, as_stream(stream), verts, normals, (int)V, faces, lay,
              p0, count, rows);
  return NERF_OK;
}

extern "C" int nerf_texture_store(const float* raw, int64_t V, const int32_t* faces, int64_t F, int texels, int64_t p0, int64_t count,
                                  uint8_t* image, void* stream) {
  TexLayout lay;
  int rc = tex_mesh_check("nerf_texture_store", V, F, texels, &lay);
  if (!rc) rc = tex_chunk_check("nerf_texture_store", lay, p0, count);
  if (rc) return rc;
  if (count == 0) return NERF_OK;
  NERF_REQUIRE(raw && image && (faces || F == 0), NERF_E_NULL, "nerf_texture_store: NULL pointer");
  NERF_REQUIRE(((uintptr_t)raw & 15) == 0, NERF_E_SHAPE, "nerf_texture_store: raw must be 16-byte aligned");
  NERF_LAUNCH("nerf_texture_store", tex_store_kernel, blocks(count, TEX_BLOCK), TEX_BLOCK, as_stream(stream), reinterpret_cast<const float4*>(raw),
              (int)V, faces, lay, p0, count, image);
  return NERF_OK;
}

extern "C" int nerf_texture_uv(int64_t F, int texels, float* uv, void* stream) {
  TexLayout lay;
  const int rc = tex_layout("nerf_texture_uv", F, texels, &lay);
  if (rc) return rc;
  if (F == 0) return NERF_OK;
  NERF_REQUIRE(uv, NERF_E_NULL, "nerf_texture_uv: NULL uv");
  NERF_LAUNCH("nerf_texture_uv", tex_uv_kernel, blocks(F, TEX_BLOCK), TEX_BLOCK, as_stream(stream), lay, uv);
  return NERF_OK;
}

extern "C" int nerf_texture_sample(const uint8_t* image, const float* verts, const float* normals, int64_t V, const int32_t* faces,
                                   int64_t F, int texels, const int32_t* sample_face, const float* bary, int64_t n, float* rgb,
                                   float* rows, void* stream) {
  TexLayout lay;
  const int rc = tex_mesh_check("nerf_texture_sample", V, F, texels, &lay);
  if (rc) return rc;
  NERF_REQUIRE(n >= 0 && n <= ((int64_t)1 << 31) - 1, NERF_E_SHAPE, "nerf_texture_sample: need 0 <= n < 2^31 (got %lld)", (long long)n);
  if (n == 0) return NERF_OK;
  NERF_REQUIRE(image && sample_face && bary && rgb, NERF_E_NULL, "nerf_texture_sample: NULL pointer");
  NERF_REQUIRE(!rows || ((faces || F == 0) && ((verts && normals) || V == 0)), NERF_E_NULL,
               "nerf_texture_sample: rows need verts, normals and faces");
  NERF_LAUNCH("nerf_texture_sample", tex_sample_kernel, blocks(n, TEX_BLOCK), TEX_BLOCK, as_stream(stream), image, verts, normals, (int)V, faces,
              lay, sample_face, bary, n, rgb, rows);
  return NERF_OK;
}
