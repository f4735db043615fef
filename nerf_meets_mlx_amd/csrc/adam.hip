// Fused multi-tensor Adam over one flat float32 parameter buffer (a21 / K9).
// HBM-bound: 28 B per parameter (read p,g,m,v; write p,m,v) = 16.7 MB per network.
#include "common.h"
#include "hash_common.h"

namespace nerf {

struct AdamArgs { float lr, b1, b2, eps, c1, c2, gscale; };

// mlx.optimizers.Adam (0.7.0): m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2;
// p = p - lr * m / (sqrt(v) + eps).  c1, c2 = 1 unless bias correction is requested.  gi: the scaled gradient; returns the new p.
__device__ __forceinline__ float adam_update(float gi, float& m, float& v, float& p, const AdamArgs& a) {
  const float mi = a.b1 * m + (1.0f - a.b1) * gi;
  const float vi = a.b2 * v + (1.0f - a.b2) * gi * gi;
  m = mi; v = vi;
  const float pn = p - a.lr * (mi * a.c1) / (sqrtf(vi * a.c2) + a.eps);
  p = pn;
  return pn;
}

// The update with (a) the gradient taken from float32 values OR from the int64 fixed-point accumulators of the
// deterministic hash-grid scatter (hash_common.h: 2^-52 units), and (b) the gradient buffer zeroed in the same pass
// (read g, write 0): the next step's scatter needs no memset launch.
// (c) SHADOW: the updated parameter is also written as fp16 into a second buffer -- the 4-byte-per-entry image of the hash
// tables that the forward gathers read (half the bytes of the float32 master pairs; the master copy stays float32).
// nerf_adam_step is <false, false, false>: it never writes gv.
template <bool FIXED, bool ZERO, bool SHADOW>
__global__ void __launch_bounds__(256) adam_kernel(float* __restrict__ p, void* __restrict__ gv, float* __restrict__ m,
                                                   float* __restrict__ v, int64_t count, AdamArgs a, _Float16* __restrict__ ph) {
  float* gf = static_cast<float*>(gv);
  long long* gi64 = static_cast<long long*>(gv);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
    float gi;
    if (FIXED) {
      const long long acc = gi64[i];
      gi = (float)((double)acc * (1.0 / NERF_HASH_FIX_SCALE)) * a.gscale;
      if (nerf_fixed_is_poisoned(acc)) gi = __builtin_nanf("");         // saturated / non-finite addend or overflowing sum (hash_common.h)
      if (ZERO) gi64[i] = 0;
    }
    else { gi = gf[i] * a.gscale; if (ZERO) gf[i] = 0.0f; }
    const float pn = adam_update(gi, m[i], v[i], p[i], a);
    if (SHADOW) ph[i] = (_Float16)pn;
  }
}

// the checks of every entry under the name `who`, and the constants of the update
static int adam_args(const char* who, const void* params, const void* grads, const void* m, const void* v, int64_t count, float lr,
                     float beta1, float beta2, float eps, int bias_correction, int step, float grad_scale, AdamArgs& a) {
  NERF_REQUIRE(params && grads && m && v, NERF_E_NULL, "%s: NULL pointer", who);
  NERF_REQUIRE(count > 0, NERF_E_SHAPE, "%s: count must be > 0", who);
  a = {lr, beta1, beta2, eps, 1.0f, 1.0f, grad_scale};
  if (bias_correction) {
    NERF_REQUIRE(step >= 1, NERF_E_SHAPE, "%s: bias correction needs step >= 1", who);
    a.c1 = 1.0f / (1.0f - powf(beta1, (float)step));
    a.c2 = 1.0f / (1.0f - powf(beta2, (float)step));
  }
  return NERF_OK;
}

}  // namespace nerf

using namespace nerf;

extern "C" int nerf_adam_step_shadow(float* params, void* grads, float* m, float* v, int64_t count, float lr, float beta1,
                                     float beta2, float eps, int bias_correction, int step, float grad_scale, int grads_fixed_point,
                                     int zero_grads, void* params_half, void* stream) {
  AdamArgs a;                                            // (errors are reported as nerf_adam_step_ex, whichever of the two was called)
  if (const int rc = adam_args("nerf_adam_step_ex", params, grads, m, v, count, lr, beta1, beta2, eps, bias_correction, step,
                               grad_scale, a)) return rc;
  _Float16* ph = static_cast<_Float16*>(params_half);
  return with_bool(grads_fixed_point != 0, [&](auto fx) {
    return with_bool(zero_grads != 0, [&](auto zr) {
      return with_bool(ph != nullptr, [&](auto sh) -> int {
        NERF_LAUNCH("nerf_adam_step_ex", (adam_kernel<decltype(fx)::value, decltype(zr)::value, decltype(sh)::value>),
                    grid_for(count, 256), 256, as_stream(stream), params, grads, m, v, count, a, ph);
        return NERF_OK;
      });
    });
  });
}

extern "C" int nerf_adam_step_ex(float* params, void* grads, float* m, float* v, int64_t count, float lr, float beta1,
                                 float beta2, float eps, int bias_correction, int step, float grad_scale, int grads_fixed_point,
                                 int zero_grads, void* stream) {
  return nerf_adam_step_shadow(params, grads, m, v, count, lr, beta1, beta2, eps, bias_correction, step, grad_scale,
                               grads_fixed_point, zero_grads, nullptr, stream);
}

extern "C" int nerf_adam_step(float* params, const float* grads, float* m, float* v, int64_t count, float lr,
                              float beta1, float beta2, float eps, int bias_correction, int step, float grad_scale,
                              void* stream) {
  AdamArgs a;
  if (const int rc = adam_args("nerf_adam_step", params, grads, m, v, count, lr, beta1, beta2, eps, bias_correction, step,
                               grad_scale, a)) return rc;
  NERF_LAUNCH("nerf_adam_step", (adam_kernel<false, false, false>), grid_for(count, 256), 256, as_stream(stream), params,
              static_cast<void*>(const_cast<float*>(grads)), m, v, count, a, static_cast<_Float16*>(nullptr));
  return NERF_OK;
}
