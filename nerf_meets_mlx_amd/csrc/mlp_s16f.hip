// The FOLDED form of the split-bf16 training kernels of the 8 x 256 view model ("train_fold"; mlp_s16.h, stream description:
// mlp_index.h, namespace LF): pack of the folded image, training forward and dZ chain with the feature layer folded into dir0.
//
// Reference: models/NeRF.py:229-236.  feature = W_F h7 + b_F has no activation (:231) and feeds only dir0's first 256 input columns,
// so  W_D [feature ; e_dir] + b_D = (W_D[:, :256] W_F) h7 + W_D[:, 256:] e_dir + (W_D[:, :256] b_F + b_D)  and, backwards,
// dZ7 = mask7([W'^T | W_A^T] [dZ_D ; d alpha]).  Per 32-sample tile the forward runs 128 fragment pairs fewer (no feature layer) and
// stores 32 KiB less (no feature blocks), the chain 128 fewer (64 + 136 become 72) and 32 KiB less (no dZ_F blocks).  The device
// code is mlp_s16_view.h's with FOLD = true; this unit exists so that its ISA is scanned on its own (Makefile) and mlp_s16.o keeps
// the kernels it always held.
#include "mlp_s16_view.h"

namespace nerf {
namespace s16 {

// The folded image (mlp_s16.h).  One thread per 16-byte lane slot of a pair, forward stream first, then one thread per float of the
// fp32 copies.  A forward-stream thread whose eight elements are W'[n][k_0 .. k_7] computes them -- eight float64 sums of 256 terms in
// index order, rounded once -- and writes them to BOTH streams (its own slot, and element by element into the transposed stream:
// fold_elem_bwd), so every element of W' is computed once and the two streams hold the same (hi, lo) bits of it.
constexpr int FOLD_PACK_PAIRS = (LF::F_TOTAL + LF::B_PADDED) * 64;
constexpr int FOLD_PACK_THREADS = FOLD_PACK_PAIRS + (LF::C_WFT_END - LF::C_WFT) + (LF::C_END - LF::C_WD1);
__global__ void __launch_bounds__(256) pack_fold_kernel(const float* __restrict__ p, bf16x8* __restrict__ img) {
  const int tid = blockIdx.x * 256 + threadIdx.x;
  bf16x8* wf = img;
  bf16x8* wb = img + (size_t)F_FRAGS * 64;               // the transposed stream starts where the unfolded one does
  float* cp = reinterpret_cast<float*>(img);
  if (tid < FOLD_PACK_PAIRS) {
    const bool fw = tid < LF::F_TOTAL * 64;
    const int t = fw ? tid : tid - LF::F_TOTAL * 64;
    const int f = t >> 6, lane = t & 63, r = lane & 31, h = lane >> 5;
    int src[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) src[j] = !fw && f >= LF::B_TOTAL ? -1 : fw ? fwd_index_fold(f, r, h, j) : bwd_index_fold(f, r, h, j);
    const bool wp = is_fold_wp(src[0]);                  // all eight elements of a lane slot are W' elements, or none is
    if (wp && !fw) return;                               // written by the forward-stream thread that computes them
    float v[8];
    if (wp) {
      const int n = fold_wp_n(src[0]);
      double acc[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = 0.0;
      for (int q = 0; q < 256; ++q) {
        const double wd = (double)p[L::P_WD + n * 283 + q];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = __builtin_fma(wd, (double)p[L::P_WF + q * 256 + fold_wp_k(src[j])], acc[j]);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (float)acc[j];
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = src[j] >= 0 ? p[src[j]] : 0.0f;
    }
    bf16x8 o[2];
    SplitBf16::pack(v, o[0], o[1]);
    bf16x8* dst = fw ? wf : wb;
    dst[(2 * f) * 64 + lane] = o[0];
    dst[(2 * f + 1) * 64 + lane] = o[1];
    if (wp) {
      __bf16* tb = reinterpret_cast<__bf16*>(wb);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const FragElem e = fold_elem_bwd(fold_wp_n(src[j]), fold_wp_k(src[j]));
        FragElem eh = e, el = e;
        eh.f = 2 * e.f; el.f = 2 * e.f + 1;
        tb[frag_elem_offset(eh)] = o[0][j];
        tb[frag_elem_offset(el)] = o[1][j];
      }
    }
    return;
  }
  int c = tid - FOLD_PACK_PAIRS;
  if (c < LF::C_WFT_END - LF::C_WFT) {                   // W_F transposed: [i][k] = W_F[k][i]
    cp[LF::C_WFT + c] = p[L::P_WF + (c & 255) * 256 + (c >> 8)];
    return;
  }
  c += LF::C_WD1 - (LF::C_WFT_END - LF::C_WFT);          // float offset in the image
  if (c >= LF::C_END) return;
  float v = 0.0f;
  if (c < LF::C_BF) { const int e = c - LF::C_WD1; v = p[L::P_WD + (e >> 8) * 283 + (e & 255)]; }
  else if (c < LF::C_BP) v = p[L::P_BF + (c - LF::C_BF)];
  else if (c < LF::C_USED) {                             // b'[n] = float32(sum_j W_D[n][j] b_F[j] + b_D[n]), b_D added last
    const int n = c - LF::C_BP;
    double acc = 0.0;
    for (int q = 0; q < 256; ++q) acc = __builtin_fma((double)p[L::P_WD + n * 283 + q], (double)p[L::P_BF + q], acc);
    v = (float)(acc + (double)p[L::P_BD + n]);
  }
  cp[c] = v;
}

int pack_folded(const float* params, void* packed_s16, hipStream_t s) {
  return launch<pack_fold_kernel>("nerf_mlp_pack (split-bf16 image, folded)", dim3((FOLD_PACK_THREADS + 255) / 256), dim3(256), 0, s, params,
                                  static_cast<bf16x8*>(packed_s16));
}

int forward_folded(const void* packed_s16, const float* bias_slots, const float* x, const float* rays, const float* z, int64_t M,
                   int n, int freq_mode, float* out, void* acts, int64_t astride16, int persistent_wgs, hipStream_t s) {
  FwdArgs a;
  a.queue = passq_slot();
  a.wf = reinterpret_cast<const bf16x8*>(packed_s16);
  a.bias = bias_slots;
  a.x = x; a.rays = rays; a.z = z; a.M = M; a.n = n; a.out = out; a.acts = acts; a.astride = astride16;
  fill_freqs(a.fr.pos, a.fr.dir, freq_mode);
  const int64_t nsuper = ((M + 31) / 32 + NW - 1) / NW;
  return with_bool(x != nullptr, [&](auto rows) {          // MODE 0: embedded rows, 1: rays + depths
    return launch<s16_fwd_kernel<decltype(rows)::value ? 0 : 1, true>>("mlp training forward (split bf16, folded)",
                                                                        dim3(persistent_grid(nsuper, persistent_wgs)), dim3(64 * NW),
                                                                        FwdRingFold::LDS_BYTES, s, a);
  });
}

int backward_chain_folded(const void* packed_s16, const void* acts, const float* d_raw, int64_t M, void* dz, int64_t astride16,
                          int64_t zstride16, int persistent_wgs, hipStream_t s) {
  BwdArgs b;
  b.queue = passq_slot();
  b.wb = reinterpret_cast<const bf16x8*>(static_cast<const char*>(packed_s16) + (size_t)F_FRAGS * 1024);     // where the unfolded one starts
  b.acts = acts; b.d_raw = d_raw; b.M = M; b.dz = dz; b.astride = astride16; b.zstride = zstride16;
  const int64_t nsuper = ((M + 31) / 32 + NW - 1) / NW;
  return launch<s16_bwd_kernel<true>>("mlp backward chain (split bf16, folded)", dim3(persistent_grid(nsuper, persistent_wgs)), dim3(64 * NW),
                                      BwdRingFold::LDS_BYTES, s, b);
}

}  // namespace s16
}  // namespace nerf
