// Post step of the factored weight gradients of the 8 x 256 view model at precision 22 ("dw_factor", job table: mlp_model.h).
//
// Reference: the adjoint of models/NeRF.py:231-236 under nn.value_and_grad.  feature = W_F h7 + b_F enters dir0 without an
// activation, so the shared dW job leaves  G[j][i] = sum_m dZ_D[j][m] H7[i][m]  (128 x 256) and  db_D[j] = sum_m dZ_D[j][m]  behind
// (mlp_frag.h: DWF_G, DWF_DB) and, exactly,
//     dW_F[k][i]          = sum_j W_D[j][k] G[j][i]                       (dZ_F = W_D[:, :256]^T dZ_D: no mask in between)
//     db_F[k]             = sum_j W_D[j][k] db_D[j]
//     dW_D[j][k], k < 256 = sum_i W_F[k][i] G[j][i] + b_F[k] db_D[j]
// Two 256-wide products of 8.4 MFLOP per call instead of two passes over the sample axis.  The weights are the values the forward
// and the dZ chain multiply with: float(hi) + float(lo) of the split-bf16 forward stream, found through the packing's own index
// functions (mlp_index.h: fwd_elem_feature / fwd_elem_dir0, the inverses of fwd_index); b_F from the fp32 bias slots.  Every sum
// (K = 128 or 256) runs in float64 in a fixed order and is rounded once: bit-reproducible, and the rounding of the post step is
// far below that of G itself.  db_D is dir0's bias gradient as it is.  Columns 256 .. 282 of dW_D (row stride 283) belong to the
// job dir0 | dirPE and are not touched.
//
// FOLD (a folded image, "train_fold": mlp_s16.h): the forward and the chain multiply with W' = W_D[:, :256] W_F, so G is exactly
// dL/dW' and the three results above are the product rule.  W_F and W_D[:, :256] are no longer streamed; the post step reads their
// fp32 masters from the copies the pack left in the image (mlp_index.h: LF::C_WFT -- W_F transposed --, LF::C_WD1, LF::C_BF).  Same
// formulas, float64 sums in index order, one rounding.
#include "common.h"
#include "launch.h"
#include "mlp_frag.h"

namespace nerf {

constexpr int DWF_ROWS = 2;                                // output rows per workgroup
constexpr int DWF_BLOCKS_F = 256 / DWF_ROWS, DWF_BLOCKS_D = 128 / DWF_ROWS;

__device__ __forceinline__ double pair_value(const __bf16* __restrict__ wf, const FragElem& e) {      // hi + lo of one stream element
  FragElem hi = e, lo = e;
  hi.f = 2 * e.f; lo.f = 2 * e.f + 1;                      // (hi, lo) fragment pairs in stream order (mlp_pack.h: SplitBf16)
  return (double)(float)wf[frag_elem_offset(hi)] + (double)(float)wf[frag_elem_offset(lo)];
}

template <bool FOLD>
__global__ void __launch_bounds__(256) mlp_dw_factor_post_kernel(const __bf16* __restrict__ wf, const float* __restrict__ bias,
                                                                 const float* __restrict__ aux, float* __restrict__ grads) {
  __shared__ double sh[256 * DWF_ROWS];                    // [K index][row of this workgroup]
  __shared__ double sdb[128];
  const int t = threadIdx.x;
  const float* G = aux + DWF_G;
  const float* dbD = aux + DWF_DB;
  const float* cp = reinterpret_cast<const float*>(wf);    // FOLD: the image's fp32 copies
  double acc[DWF_ROWS];
#pragma unroll
  for (int q = 0; q < DWF_ROWS; ++q) acc[q] = 0.0;
  if (blockIdx.x < DWF_BLOCKS_F) {
    // DWF_ROWS rows of dW_F from k0 on (thread = column i) and their db_F
    const int k0 = DWF_ROWS * blockIdx.x;
    for (int e = t; e < 128 * DWF_ROWS; e += 256) {        // sh[j][q] = W_D[j][k0 + q]
      const int j = e / DWF_ROWS, q = e % DWF_ROWS;
      sh[e] = FOLD ? (double)cp[LF::C_WD1 + j * 256 + k0 + q] : pair_value(wf, fwd_elem_dir0(j, k0 + q));
    }
    if (t < 128) sdb[t] = (double)dbD[t];
    __syncthreads();
    for (int j = 0; j < 128; ++j) {
      const double g = (double)G[j * 256 + t];
#pragma unroll
      for (int q = 0; q < DWF_ROWS; ++q) acc[q] = __builtin_fma(sh[j * DWF_ROWS + q], g, acc[q]);
    }
#pragma unroll
    for (int q = 0; q < DWF_ROWS; ++q) grads[L::P_WF + (k0 + q) * 256 + t] = (float)acc[q];
    if (t < DWF_ROWS) {
      double b = 0.0;
      for (int j = 0; j < 128; ++j) b = __builtin_fma(sh[j * DWF_ROWS + t], sdb[j], b);
      grads[L::P_BF + k0 + t] = (float)b;
    }
  } else {
    // DWF_ROWS rows of dW_D from j0 on, columns 0 .. 255 (thread = column k)
    const int j0 = DWF_ROWS * (blockIdx.x - DWF_BLOCKS_F);
    for (int e = t; e < 256 * DWF_ROWS; e += 256) {        // sh[i][q] = G[j0 + q][i]
      const int q = e / 256, i = e % 256;
      sh[i * DWF_ROWS + q] = (double)G[(j0 + q) * 256 + i];
    }
    __syncthreads();
    if constexpr (FOLD) {
      for (int i = 0; i < 256; ++i) {
        const double w = (double)cp[LF::C_WFT + i * 256 + t];      // W_F[t][i]
#pragma unroll
        for (int q = 0; q < DWF_ROWS; ++q) acc[q] = __builtin_fma(w, sh[i * DWF_ROWS + q], acc[q]);
      }
    } else
    for (int ks = 0; ks < 16; ++ks) {
      for (int h = 0; h < 2; ++h) {
        // the eight elements of lane (t & 31, h) of k-step ks: W_F[t][kperm(ks, h, 0 .. 7)], 16 contiguous bytes per part
        const FragElem e0 = fwd_elem_feature(t, kperm(ks, h, 0));
        FragElem eh = e0, el = e0;
        eh.f = 2 * e0.f; el.f = 2 * e0.f + 1;
        const bf16x8 vh = *reinterpret_cast<const bf16x8*>(wf + frag_elem_offset(eh));
        const bf16x8 vl = *reinterpret_cast<const bf16x8*>(wf + frag_elem_offset(el));
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
          const double w = (double)(float)vh[jj] + (double)(float)vl[jj];
          const int i = kperm(ks, h, jj);
#pragma unroll
          for (int q = 0; q < DWF_ROWS; ++q) acc[q] = __builtin_fma(w, sh[i * DWF_ROWS + q], acc[q]);
        }
      }
    }
    const double bf = (double)(FOLD ? cp[LF::C_BF + t] : bias[L::BI_FEAT + t]);
#pragma unroll
    for (int q = 0; q < DWF_ROWS; ++q) grads[L::P_WD + (j0 + q) * 283 + t] = (float)__builtin_fma(bf, (double)dbD[j0 + q], acc[q]);
    if (t < DWF_ROWS) grads[L::P_BD + j0 + t] = dbD[j0 + t];      // db_D itself: the shared job's bias sums are dir0's bias gradient
  }
}

int launch_dw_factor_post(const void* packed_s16, const float* bias_slots, const float* aux, float* grads, bool fold, hipStream_t s) {
  return with_bool(fold, [&](auto fd) {
    return launch<mlp_dw_factor_post_kernel<decltype(fd)::value>>("mlp dW post step (factored feature / dir0)", dim3(DWF_BLOCKS_F + DWF_BLOCKS_D),
                                                                  dim3(256), 0, s, static_cast<const __bf16*>(packed_s16), bias_slots, aux, grads);
  });
}

}  // namespace nerf
