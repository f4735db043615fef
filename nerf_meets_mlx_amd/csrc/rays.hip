// Ray generation, pixel selection, row gather, NDC warp  (SURVEY 8a rows a1-a4, K1/K12).
// HBM-bound, one thread per ray; 44 B written per ray, nothing read but the index.
#include "common.h"
#include "perm.h"

namespace nerf {

__global__ void perm_kernel(int64_t* out, int64_t n, uint64_t domain, uint64_t offset, PermKey key) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = (int64_t)perm_value(offset, i, domain, key);
}

struct Cam { double fx, fy, cx, cy; float r[9]; float t[3]; };
static Cam make_cam(const double* K, const float* c2w) {
  Cam cam;
  cam.fx = K[0]; cam.fy = K[4]; cam.cx = K[2]; cam.cy = K[5];
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b) cam.r[3 * a + b] = c2w[4 * a + b];
    cam.t[a] = c2w[4 * a + 3];
  }
  return cam;
}

__device__ __forceinline__ void write_ray(int64_t i, int64_t p, int W, const Cam& cam, float near, float far,
                                          float* __restrict__ rays, int64_t* __restrict__ coords) {
  const int64_t row = p / W, col = p - row * W;
  // dirs = [(i-cx)/fx, -(j-cy)/fy, -1], i = column, j = row, integer pixel centres
  const double dx = ((double)col - cam.cx) / cam.fx;
  const double dy = -((double)row - cam.cy) / cam.fy;
  const double dz = -1.0;
  double d[3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
    d[a] = dx * (double)cam.r[3 * a + 0] + dy * (double)cam.r[3 * a + 1] + dz * (double)cam.r[3 * a + 2];
  const float fx_ = (float)d[0], fy_ = (float)d[1], fz_ = (float)d[2];
  // viewdirs = d / |d| on the float32 d (entrypoints/__test_nerf.py:62-64 works on the f32 array), normalised in float64 and
  // rounded once: within 1 ulp of the exact unit vector (float32 arithmetic here erred by up to 2.6 ulp)
  const double x = fx_, y = fy_, z = fz_;
  const double inv = 1.0 / sqrt(x * x + y * y + z * z);
  float* o = rays + i * NERF_RAY_STRIDE;
  o[0] = cam.t[0]; o[1] = cam.t[1]; o[2] = cam.t[2];
  o[3] = fx_; o[4] = fy_; o[5] = fz_;
  o[6] = near; o[7] = far;
  o[8] = (float)(x * inv); o[9] = (float)(y * inv); o[10] = (float)(z * inv);
  if (coords) { coords[2 * i] = row; coords[2 * i + 1] = col; }
}

__global__ void ray_gen_kernel(const int64_t* __restrict__ idx, int64_t n, int W, Cam cam, float near, float far,
                               float* __restrict__ rays, int64_t* __restrict__ coords) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    write_ray(i, idx ? idx[i] : i, W, cam, near, far, rays, coords);
}

// One training batch in one launch (entrypoints/__test_nerf.py:213-236 + 60-82): the i-th of n distinct pixels of the
// keyed permutation, its ray, and its target colour from the resident image -- perm_kernel, ray_gen_kernel and
// gather_rows_kernel back to back, with the same arithmetic (bit-identical outputs), as ONE kernel: at N_rand = 1024 an
// iteration is ~1.3 ms and each five-microsecond launch shows.
// Px = float: an RGB image [H*W, 3], three scalar copies per pixel; Px = float4: a straight RGBA image [H*W, 4], the same
// permutation and rays, one 16-byte copy per pixel.
template <class Px>
__global__ void sample_batch_kernel(int64_t n, uint64_t domain, uint64_t offset, PermKey key, int W, Cam cam, float near,
                                    float far, const Px* __restrict__ image, float* __restrict__ rays,
                                    Px* __restrict__ target, int64_t* __restrict__ idx_out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t v = perm_value(offset, i, domain, key);
    write_ray(i, (int64_t)v, W, cam, near, far, rays, nullptr);
    if constexpr (std::is_same<Px, float4>::value) target[i] = image[v];
    else { target[3 * i] = image[3 * v]; target[3 * i + 1] = image[3 * v + 1]; target[3 * i + 2] = image[3 * v + 2]; }
    if (idx_out) idx_out[i] = (int64_t)v;
  }
}

// An index outside [0, n_src) never reads: its output row is NaN (the launch is asynchronous, so it cannot fail)
__global__ void gather_rows_kernel(const float* __restrict__ src, int64_t n_src, const int64_t* __restrict__ idx,
                                   int64_t n, int C, float* __restrict__ out) {
  const int64_t total = n * C;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t / C; const int c = (int)(t - i * C);
    const int64_t row = idx[i];
    out[t] = (row >= 0 && row < n_src) ? src[row * C + c] : __builtin_nanf("");
  }
}

__global__ void ndc_kernel(float* rays, int64_t n, float sx, float sy, float near) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float* r = rays + i * NERF_RAY_STRIDE;
    float ox = r[0], oy = r[1], oz = r[2], dx = r[3], dy = r[4], dz = r[5];
    const float tn = -(near + oz) / dz;
    ox += tn * dx; oy += tn * dy; oz += tn * dz;
    r[0] = sx * (ox / oz); r[1] = sy * (oy / oz); r[2] = 1.0f + 2.0f * near / oz;
    r[3] = sx * (dx / dz - ox / oz); r[4] = sy * (dy / dz - oy / oz); r[5] = -2.0f * near * (1.0f / oz);
  }
}

}  // namespace nerf

using namespace nerf;

extern "C" int nerf_pixel_permutation(int64_t* out_idx, int64_t n, int64_t domain, uint64_t seed, uint64_t offset,
                                      void* stream) {
  NERF_REQUIRE(out_idx, NERF_E_NULL, "nerf_pixel_permutation: out_idx is NULL");
  NERF_REQUIRE(n >= 0 && domain >= 1 && (int64_t)offset + n <= domain, NERF_E_SHAPE,
               "nerf_pixel_permutation: need offset+n <= domain (n=%lld domain=%lld)", (long long)n, (long long)domain);
  if (n == 0) return NERF_OK;
  NERF_LAUNCH("nerf_pixel_permutation", perm_kernel, grid_for(n, 256), 256, as_stream(stream), out_idx, n, (uint64_t)domain,
              offset, make_key(seed, (uint64_t)domain));
  return NERF_OK;
}

extern "C" int nerf_ray_gen(const int64_t* pixel_idx, int64_t n, int H, int W, const double* K, const float* c2w,
                            float near, float far, float* rays, int64_t* coords, void* stream) {
  NERF_REQUIRE(H > 0 && W > 0 && n >= 0, NERF_E_SHAPE, "nerf_ray_gen: bad H/W/n");
  if (n == 0) return NERF_OK;
  NERF_REQUIRE(K && c2w && rays, NERF_E_NULL, "nerf_ray_gen: K/c2w/rays is NULL");
  NERF_REQUIRE(pixel_idx || n == (int64_t)H * W, NERF_E_SHAPE, "nerf_ray_gen: pixel_idx NULL requires n == H*W");
  NERF_LAUNCH("nerf_ray_gen", ray_gen_kernel, grid_for(n, 256), 256, as_stream(stream), pixel_idx, n, W, make_cam(K, c2w), near,
              far, rays, coords);
  return NERF_OK;
}

// both sample-batch entries; Px as in sample_batch_kernel (float4 rows must be 16-byte aligned)
template <class Px>
static int sample_batch(const char* who, int64_t n, int H, int W, uint64_t seed, uint64_t offset, const double* K,
                        const float* c2w, float near, float far, const float* image, float* rays, float* target,
                        int64_t* pixel_idx, void* stream) {
  NERF_REQUIRE(H > 0 && W > 0 && n >= 0, NERF_E_SHAPE, "%s: bad H/W/n", who);
  NERF_REQUIRE((int64_t)offset + n <= (int64_t)H * W, NERF_E_SHAPE, "%s: need offset+n <= H*W (n=%lld H*W=%lld)", who,
               (long long)n, (long long)H * W);
  if (n == 0) return NERF_OK;
  NERF_REQUIRE(K && c2w && image && rays && target, NERF_E_NULL, "%s: NULL pointer", who);
  if (std::is_same<Px, float4>::value)
    NERF_REQUIRE(((reinterpret_cast<uintptr_t>(image) | reinterpret_cast<uintptr_t>(target)) & 15) == 0, NERF_E_SHAPE,
                 "%s: image / target must be 16-byte aligned", who);
  const uint64_t domain = (uint64_t)H * (uint64_t)W;
  NERF_LAUNCH(who, sample_batch_kernel<Px>, grid_for(n, 256), 256, as_stream(stream), n, domain, offset, make_key(seed, domain), W,
              make_cam(K, c2w), near, far, reinterpret_cast<const Px*>(image), rays, reinterpret_cast<Px*>(target), pixel_idx);
  return NERF_OK;
}

extern "C" int nerf_sample_batch(int64_t n, int H, int W, uint64_t seed, uint64_t offset, const double* K,
                                 const float* c2w, float near, float far, const float* image, float* rays,
                                 float* target, int64_t* pixel_idx, void* stream) {
  return sample_batch<float>("nerf_sample_batch", n, H, W, seed, offset, K, c2w, near, far, image, rays, target, pixel_idx, stream);
}

extern "C" int nerf_sample_batch_rgba(int64_t n, int H, int W, uint64_t seed, uint64_t offset, const double* K,
                                      const float* c2w, float near, float far, const float* image, float* rays,
                                      float* target, int64_t* pixel_idx, void* stream) {
  return sample_batch<float4>("nerf_sample_batch_rgba", n, H, W, seed, offset, K, c2w, near, far, image, rays, target, pixel_idx,
                              stream);
}

extern "C" int nerf_gather_rows(const float* src, int64_t n_src, const int64_t* idx, int64_t n, int channels,
                                float* out, void* stream) {
  NERF_REQUIRE(n >= 0 && channels > 0, NERF_E_SHAPE, "nerf_gather_rows: bad sizes");
  if (n == 0) return NERF_OK;
  NERF_REQUIRE(src && idx && out, NERF_E_NULL, "nerf_gather_rows: NULL pointer");
  NERF_REQUIRE(n_src > 0, NERF_E_SHAPE, "nerf_gather_rows: empty source");
  NERF_LAUNCH("nerf_gather_rows", gather_rows_kernel, grid_for(n * channels, 256), 256, as_stream(stream), src, n_src, idx, n,
              channels, out);
  return NERF_OK;
}

extern "C" int nerf_ndc_rays(float* rays, int64_t n, int H, int W, float focal, float near, void* stream) {
  if (n <= 0) return NERF_OK;
  NERF_REQUIRE(rays, NERF_E_NULL, "nerf_ndc_rays: rays is NULL");
  NERF_LAUNCH("nerf_ndc_rays", ndc_kernel, grid_for(n, 256), 256, as_stream(stream), rays, n, -focal / (0.5f * W),
              -focal / (0.5f * H), near);
  return NERF_OK;
}
