// The split-bf16 fused configs[4] query with per-level weights (nerf_ngp_query_fused_lw at precision 22): the LW = true
// instantiations of mlp_s16x_small.h's forward kernel, in a translation unit of their own (built and ISA-scanned like
// mlp_s16x.hip: NERF_DMA_CLOBBER_M0, no scratch).
#include "mlp_s16x_small.h"

namespace nerf {
namespace s16x {

int small_forward_lw(const SmallArgs& a, dim3 grid, hipStream_t s) {
  return with_bool(a.acts != nullptr, [&](auto store) {
    return launch<s16_small_fwd_kernel<decltype(store)::value, true, true>>("mlp forward (2x64 model, split bf16, level weights)", grid, dim3(512),
                                                                            SM_LDS_BYTES, s, a);
  });
}

}  // namespace s16x
}  // namespace nerf
