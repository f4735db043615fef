// Split-fp16 ("precision 22") inference forward of the fused 8 x 256 chain (mlp22.hip): interface used by the C ABI
// entry points of mlp.hip for a model whose nerf_mlp_arch.precision is 22, and the description of its weight stream (pure integer
// arithmetic without a HIP dependency: tests/f22_stream_check.cpp walks it on the host).
//
// Every float32 operand x of the reference's GEMMs (models/NeRF.py:201-243) is carried as TWO fp16 numbers,
// x = hi + lo * 2^-11 with hi = fp16(x), lo = fp16((x - hi) * 2^11): 22 significand bits.  A product w x is evaluated as
// w_hi x_hi + 2^-11 (w_hi x_lo + w_lo x_hi) -- three v_mfma_f32_16x16x32_f16 per float32 product, fp32 accumulate, the
// dropped w_lo x_lo term is 2^-22 relative -- so the matrix pipe runs at 1/3 of its fp16 rate instead of the 1/16 of the
// fp32 MFMA, at float32-class accuracy (measured <= 2e-6 of the output scale against the fp32 oracle).
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>
#include "mlp_index.h"

// 1 (the shipped form): the feature layer is folded into dir0 when the image is packed.  feature = W_F h7 + b_F has no activation
// (models/NeRF.py:231) and dir0's first 256 input columns are its only consumer, so
//     W_D [feature ; e_dir] + b_D = (W_D1 W_F) h7 + W_D[:, 256:] e_dir + (W_D1 b_F + b_D),     W_D1 = W_D[:, :256]
// and the stream carries W' = W_D1 W_F (128 x 256) where it carried W_F (256 x 256) and W_D1: 1044 instead of 1172 fragment pairs
// per pass.  0: the stream and the kernel of the unfolded form (A/B builds).  A compile-time switch on purpose: a packed image holds
// one form, and a run-time option could disagree with it.
#ifndef NERF_F22_FOLD
#define NERF_F22_FOLD 1
#endif

namespace nerf {
namespace f22 {

// packed image: forward stream of (hi, lo) fragment PAIRS in consumption order (2 x F_PAIRS fragments of 1 KiB, padded to whole
// 32-fragment ring chunks: F_STREAM) inside a region of F_PADDED fragments (the unfolded form's size: the image keeps its layout
// whichever form it holds; the rest of the region is zero) | fp32 bias slots (same slot numbering as the bf16 image)
// pair offsets: trunk pos0..pos7 as in the bf16 16x16x32 stream (mlp_layout.h, L16), then
//     folded:    alpha head 8 | dir0' 8 n-tiles x (8 k-steps of W' + the direction encoding's k-step) | rgb head 4
//     unfolded:  feature 128 | alpha head 8 | dir0 72 | rgb head 4
constexpr int P_L0 = 0, P_L1 = 32, P_L5 = 544, P_L6 = 704, P_L7 = 832, P_HEADS = 960;
#if NERF_F22_FOLD
constexpr int P_ALPHA = P_HEADS, P_DIR = P_ALPHA + 8, P_RGB = P_DIR + 72, F_PAIRS = P_RGB + 4;              // 1044
#else
constexpr int P_FEAT = P_HEADS, P_ALPHA = P_FEAT + 128, P_DIR = P_ALPHA + 8, P_RGB = P_DIR + 72, F_PAIRS = P_RGB + 4;     // 1172
#endif
constexpr int F_CHUNK = 32;                                                     // fragments per ring chunk (mlp_ring.h, RING_CHUNK)
constexpr int F_FRAGS = 2 * F_PAIRS, F_STREAM = (F_FRAGS + F_CHUNK - 1) / F_CHUNK * F_CHUNK, CHUNKS = F_STREAM / F_CHUNK;
constexpr int F_PADDED = 2368, BIAS_FLOATS = 2496;
constexpr int64_t PACKED_BYTES = (int64_t)F_PADDED * 1024 + (int64_t)BIAS_FLOATS * 4;
static_assert(F_STREAM <= F_PADDED && F_FRAGS % 4 == 0, "f22 stream layout");

#if NERF_F22_FOLD
// What the packing puts into element j (of 8) of lane (i = lane & 15: row of the 16-row tile, g = lane >> 4) of fragment pair fp:
// p >= 0: master parameter p (mlp_params.h); SRC_ZERO: padding; SRC_FOLD: element (n, k) of W' = W_D[:, :256] W_F
constexpr int SRC_ZERO = -1, SRC_FOLD = -2;
struct Src { int p, n, k; };
__host__ __device__ constexpr Src src_param(int p) { return Src{p, 0, 0}; }
__host__ __device__ constexpr Src src_pos_chan(int row_base, int ks, int g, int j) {          // an encoding k-step of pos0 / pos5
  return pos_chan16(ks, g, j) >= 0 ? src_param(row_base + pos_chan16(ks, g, j)) : Src{SRC_ZERO, 0, 0};
}
__host__ __device__ constexpr Src stream_src(int fp, int i, int g, int j) {
  if (fp < P_L1) return src_pos_chan(L::P_W0 + (16 * (fp / 2) + i) * 63, fp % 2, g, j);
  if (fp < P_L5 || (fp >= P_L6 && fp < P_HEADS)) {                                            // pos1..pos4, pos6, pos7
    const int q = fp < P_L5 ? fp - P_L1 : fp - P_L6, l = (fp < P_L5 ? 1 : 6) + q / 128, r = q % 128;
    return src_param(L::pw(l) + (16 * (r / 8) + i) * 256 + kperm16(r % 8, g, j));
  }
  if (fp < P_L6) {                                                                            // pos5: [encoding 2 k-steps | h 8]
    const int q = fp - P_L5, n = 16 * (q / 10) + i, ks = q % 10;
    return ks < 2 ? src_pos_chan(L::P_W5 + n * 319, ks, g, j) : src_param(L::P_W5 + n * 319 + 63 + kperm16(ks - 2, g, j));
  }
  if (fp < P_DIR) return i == 0 ? src_param(L::P_WA + kperm16(fp - P_ALPHA, g, j)) : Src{SRC_ZERO, 0, 0};
  if (fp < P_RGB) {                                                                           // dir0': [h7 8 k-steps | direction encoding]
    const int q = fp - P_DIR, n = 16 * (q / 9) + i, ks = q % 9;
    if (ks < 8) return Src{SRC_FOLD, n, kperm16(ks, g, j)};
    return dir_chan16(g, j) >= 0 ? src_param(L::P_WD + n * 283 + 256 + dir_chan16(g, j)) : Src{SRC_ZERO, 0, 0};
  }
  if (fp < F_PAIRS) return i < 3 ? src_param(L::P_WR + i * 128 + kperm16(fp - P_RGB, g, j)) : Src{SRC_ZERO, 0, 0};
  return Src{SRC_ZERO, 0, 0};
}
#endif

#ifdef __HIPCC__
extern int g_tiles;    // "f22_tiles" (mlp22.hip)
int pack(const float* params, void* packed22, hipStream_t s);
// x != nullptr: embedded rows [M,90]; else rays [B,11] + z [B,n] with the encodings evaluated in the kernel.
// persistent_wgs: workgroups of the persistent launch (one per CU)
int forward(const void* packed22, const float* x, const float* rays, const float* z, int64_t M, int n, int freq_mode,
            float* out, int persistent_wgs, hipStream_t s);
#endif

}  // namespace f22
}  // namespace nerf
