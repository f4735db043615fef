// The split-bf16 fused configs[4] query with per-level weights (nerf_ngp_query_fused_lw at precision 22): the LW = true
// instantiations of mlp_s16x_small.h's forward kernel, in a translation unit of their own (built and ISA-scanned like
// mlp_s16x.hip: NERF_DMA_CLOBBER_M0, no scratch).
#include "mlp_s16x_small.h"

namespace nerf {
namespace s16x {

int small_forward_lw(const SmallArgs& a, dim3 grid, hipStream_t s) {
  static DevOnce once[2];
  auto want = [](auto kernel, DevOnce& o) {
    o.run([&] { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, SM_LDS_BYTES); });
  };
  if (a.acts) { want(s16_small_fwd_kernel<true, true, true>, once[0]); hipLaunchKernelGGL((s16_small_fwd_kernel<true, true, true>), grid, dim3(512), SM_LDS_BYTES, s, a); }
  else { want(s16_small_fwd_kernel<false, true, true>, once[1]); hipLaunchKernelGGL((s16_small_fwd_kernel<false, true, true>), grid, dim3(512), SM_LDS_BYTES, s, a); }
  return check_launch("mlp forward (2x64 model, split bf16, level weights)");
}

}  // namespace s16x
}  // namespace nerf
