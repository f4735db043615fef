// nerf_mlp_pack, once: fp32 master parameters -> the 32x32x16 weight fragment streams of a model (+ its fp32 bias slots).
// One thread per 16-byte lane slot of a fragment, forward stream first, then one thread per bias slot: thread -> (fragment, lane),
// eight source values through the model's index maps, convert, store.  S describes the model (ViewPack in mlp_index.h, ImgPack /
// SmallPack in mlp_arch2.h; a unit whose stream is padded differently derives from one and overrides the count), PK the
// conversion: CvtBf16 (mlp_frag.h) = one bf16 fragment at f, s16::SplitBf16 (mlp_s16_dev.h) = a (hi, lo) pair at 2 f, 2 f + 1.
#pragma once
#include "mlp_frag.h"

namespace nerf {

template <class S, bool BIAS>
constexpr int pack_threads() { return (S::F_PADDED + S::B_PADDED) * 64 + (BIAS ? S::BI_TOTAL : 0); }
template <class S, bool BIAS>
constexpr int pack_blocks() { return (pack_threads<S, BIAS>() + 255) / 256; }

template <class S, class PK, bool BIAS>
__device__ __forceinline__ void pack_streams(int tid, const float* __restrict__ p, bf16x8* __restrict__ wf, bf16x8* __restrict__ wb,
                                             float* __restrict__ bias, int out_ch) {
  constexpr int nf = S::F_PADDED * 64, nb = S::B_PADDED * 64;
  if (tid < nf + nb) {
    const bool fw = tid < nf;
    const int t = fw ? tid : tid - nf;
    const int f = t >> 6, lane = t & 63, r = lane & 31, h = lane >> 5;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int i = pack_index<S>(fw, f, r, h, j, out_ch);
      v[j] = i >= 0 ? p[i] : 0.0f;
    }
    bf16x8 o[PK::FRAGS];
    if constexpr (PK::FRAGS == 1) PK::pack(v, o[0]);
    else PK::pack(v, o[0], o[1]);
    bf16x8* dst = fw ? wf : wb;
#pragma unroll
    for (int k = 0; k < PK::FRAGS; ++k) dst[(PK::FRAGS * f + k) * 64 + lane] = o[k];
  } else if (BIAS && tid < nf + nb + S::BI_TOTAL) {
    const int s = tid - nf - nb, i = S::bias(s, out_ch);
    bias[s] = i >= 0 ? p[i] : 0.0f;
  }
}

template <class S, class PK, bool BIAS>
__global__ void __launch_bounds__(256) pack_streams_kernel(const float* __restrict__ p, bf16x8* __restrict__ wf, bf16x8* __restrict__ wb,
                                                           float* __restrict__ bias, int out_ch) {
  pack_streams<S, PK, BIAS>(blockIdx.x * 256 + threadIdx.x, p, wf, wb, bias, out_ch);
}

}  // namespace nerf
