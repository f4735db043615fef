// Which master parameter sits where in the 32x32x16 weight fragment streams of the 8 x 256 view model, and back.  Pure integer
// arithmetic without a HIP dependency, shared by host and device: nerf_mlp_pack fills the streams through fwd_index / bwd_index
// (mlp_pack.h, by way of ViewPack below), the post step of the factored weight gradients (mlp_dwf.hip) finds W_F and W_D in the packed
// split-bf16 image through fwd_elem, and a CPU test walks both directions against each other (tests/frag_index_check.cpp).
#pragma once
#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif
#include "mlp_params.h"

namespace nerf {

namespace L {
// forward weight stream, 1 KiB fragments in consumption order
constexpr int F_L0 = 0, F_L1 = 32, F_L5 = 544, F_L6 = 704, F_L7 = 832, F_FA = 960, F_DIR = 1104, F_RGB = 1176;
constexpr int F_TOTAL = 1184;
// backward (transposed) weight stream
constexpr int B_RGB = 0, B_DIR = 4, B_FA = 68, B_L7 = 204, B_L6 = 332, B_L5 = 460, B_L4 = 588;
constexpr int B_TOTAL = 1100, B_PADDED = 1120;    // padded with zero fragments to whole 32-fragment ring chunks
// fp32 bias slots: pos l at 256 l, then feature, alpha (one row of a 32-row tile), dir0, rgb (three rows)
constexpr int BI_FEAT = 2048, BI_ALPHA = 2304, BI_DIR = 2336, BI_RGB = 2464, BI_TOTAL = 2496;
}  // namespace L

// element j of lane half h in k-step ks  <->  feature index
__host__ __device__ constexpr int kperm(int ks, int h, int j) { return 16 * ks + 8 * (j >> 2) + 4 * h + (j & 3); }
// ... and back: feature index kk = kperm(kperm_ks(kk), kperm_h(kk), kperm_j(kk))
__host__ __device__ constexpr int kperm_ks(int kk) { return kk >> 4; }
__host__ __device__ constexpr int kperm_h(int kk) { return (kk >> 2) & 1; }
__host__ __device__ constexpr int kperm_j(int kk) { return 4 * ((kk >> 3) & 1) + (kk & 3); }

// the 16x16x32 forward streams (bf16 render kernel of mlp.hip, split-fp16 forward of mlp22.hip): element j of lane group g in k-step ks
__host__ __device__ constexpr int kperm16(int ks, int g, int j) { return 32 * ks + 16 * (j >> 2) + 4 * g + (j & 3); }
// Which embedding channel sits in element j of lane group g in the encoding k-steps.  The order is ours to choose
// (the packed weights follow it), so it is chosen to make the per-element (sin | cos, x | y | z) pattern the same in
// all four lane groups -- only the frequency differs, three per-lane registers -- instead of a table lookup and four
// selects per element.  Position (63 channels, 2 k-steps = slots 8 ks + j): slots 0-11 = bands 2g, 2g+1 as
// (sin xyz, cos xyz); slots 12-14 = band 8 + (g>>1), sin for even g / cos for odd g, xyz; slot 15 = identity
// channel g (zero pad for g = 3).  Direction (27 channels, 1 k-step): j 0-5 = band g, j 6 = identity g, j 7 = pad.
__host__ __device__ constexpr int pos_chan16(int ks, int g, int j) {
  const int sl = 8 * ks + j;
  if (sl < 12) return 3 + 6 * (2 * g + sl / 6) + (sl % 6);
  if (sl < 15) return 3 + 6 * (8 + (g >> 1)) + 3 * (g & 1) + (sl - 12);
  return g < 3 ? g : -1;
}
__host__ __device__ constexpr int dir_chan16(int g, int j) {
  if (j < 6) return 3 + 6 * g + j;
  return (j == 6 && g < 3) ? g : -1;
}

// ------------------------------------------------------------------------------------------
// weight packing sources: offset of the master parameter that sits in element j of lane (r, h) of fragment f; -1 = zero padding
// ------------------------------------------------------------------------------------------
__host__ __device__ constexpr int fwd_index(int f, int r, int h, int j) {
  if (f < L::F_L1) {                                   // pos0: K space 64 (63 + pad)
    const int nt = f / 4, ks = f % 4;
    const int kk = kperm(ks, h, j);
    return kk < 63 ? L::P_W0 + (32 * nt + r) * 63 + kk : -1;
  }
  if (f < L::F_L5) {                                   // pos1..pos4
    const int l = 1 + (f - L::F_L1) / 128, g = (f - L::F_L1) % 128;
    const int nt = g / 16, ks = g % 16;
    return L::pw(l) + (32 * nt + r) * 256 + kperm(ks, h, j);
  }
  if (f < L::F_L6) {                                   // pos5: [PE(64), H4(256)] vs W5[256][319]
    const int g = f - L::F_L5;
    const int nt = g / 20, ks = g % 20;
    const int kk = kperm(ks, h, j), n = 32 * nt + r;
    if (kk < 64) return kk < 63 ? L::P_W5 + n * 319 + kk : -1;
    return L::P_W5 + n * 319 + 63 + (kk - 64);
  }
  if (f < L::F_FA) {                                   // pos6, pos7
    const int l = 6 + (f - L::F_L6) / 128, g = (f - L::F_L6) % 128;
    const int nt = g / 16, ks = g % 16;
    return L::pw(l) + (32 * nt + r) * 256 + kperm(ks, h, j);
  }
  if (f < L::F_DIR) {                                  // feature (8 tiles) + alpha (tile 8, row 0)
    const int g = f - L::F_FA;
    const int nt = g / 16, ks = g % 16;
    const int kk = kperm(ks, h, j);
    if (nt < 8) return L::P_WF + (32 * nt + r) * 256 + kk;
    return r == 0 ? L::P_WA + kk : -1;
  }
  if (f < L::F_RGB) {                                  // dir0: [feature(256), dirPE(27+5 pad)] vs WD[128][283]
    const int g = f - L::F_DIR;
    const int nt = g / 18, ks = g % 18;
    const int kk = kperm(ks, h, j), n = 32 * nt + r;
    if (kk < 256) return L::P_WD + n * 283 + kk;
    return (kk - 256) < 27 ? L::P_WD + n * 283 + kk : -1;
  }
  const int ks = f - L::F_RGB;                         // rgb: rows 0..2 of one tile, K = 128
  return r < 3 ? L::P_WR + r * 128 + kperm(ks, h, j) : -1;
}

// transposed stream: A rows = INPUT feature (32 kt + r), k index = OUTPUT feature nn
__host__ __device__ constexpr int bwd_index(int f, int r, int h, int j) {
  if (f < L::B_DIR) {                                  // rgb^T: 4 tiles of H_d, one k-step (rows 0..2)
    const int nn = kperm(0, h, j);
    return nn < 3 ? L::P_WR + nn * 128 + 32 * f + r : -1;
  }
  if (f < L::B_FA) {                                   // dir0^T, feature columns only: 8 tiles x 8 k-steps
    const int g = f - L::B_DIR, kt = g / 8, ns = g % 8;
    return L::P_WD + kperm(ns, h, j) * 283 + 32 * kt + r;
  }
  if (f < L::B_L7) {                                   // [feature; alpha]^T: 8 tiles x 17 k-steps
    const int g = f - L::B_FA, kt = g / 17, ns = g % 17;
    const int nn = kperm(ns, h, j);
    if (ns < 16) return L::P_WF + nn * 256 + 32 * kt + r;
    return nn == 256 ? L::P_WA + 32 * kt + r : -1;
  }
  const int g = f - L::B_L7, li = g / 128, q = g % 128, kt = q / 16, ns = q % 16;   // pos7, 6, 5, 4, 3, 2, 1
  const int l = 7 - li, nn = kperm(ns, h, j), row = 32 * kt + r;
  if (l == 5) return L::P_W5 + nn * 319 + 63 + row;
  return L::pw(l) + nn * 256 + row;
}

// ------------------------------------------------------------------------------------------
// The folded form of the split-bf16 training image ("train_fold", mlp_s16.hip).  feature = W_F h7 + b_F has no activation
// (models/NeRF.py:231), so dir0 reads h7 through  W' = W_D[:, :256] W_F  (128 x 256) with bias  b' = W_D[:, :256] b_F + b_D:
//   forward stream     trunk (unchanged) | alpha head 16 | dir0' = [W' | W_D[:, 256:]] 4 x 18 | rgb 8        = 1056 pairs
//   transposed stream  rgb^T 4 | [W'^T | W_A^T] 8 x 9 (input [dZ_D | d alpha]) | trunk (unchanged)           =  972 pairs
// Each stream is 128 pairs (256 KiB) shorter than the unfolded one; the image keeps its size, and the freed bytes hold the fp32
// masters the post step of the factored weight gradients needs (mlp_dwf.hip): LF::C_* below.  A source is a master parameter
// offset (>= 0), zero padding (-1) or element (n, k) of W' (fold_wp(n, k) <= -2), which nerf_mlp_pack computes.
// ------------------------------------------------------------------------------------------
namespace LF {
constexpr int F_A = L::F_FA, F_DIR = F_A + 16, F_RGB = F_DIR + 72, F_TOTAL = F_RGB + 8;         // 960, 976, 1048, 1056
constexpr int B_RGB = 0, B_DA = 4, B_L7 = B_DA + 72, B_TOTAL = B_L7 + 7 * 128;                  // 0, 4, 76, 972
constexpr int B_PADDED = 976;                          // pairs: 1952 fragments = 61 whole ring chunks
constexpr int B_SHIFT = L::B_L7 - B_L7;                // trunk fragment of the unfolded stream = folded + B_SHIFT
// fp32 copies in the bytes the shorter streams free, as float offsets from the start of the split-bf16 image (unfolded pair streams:
// 2 x L::F_TOTAL fragments forward, 2 x 1104 transposed; a fragment is 256 floats).  Behind the forward stream: W_F TRANSPOSED
// ([i][k] = W_F[k][i], 256 x 256: the post step reads it along k).  Behind the transposed stream: W_D[:, :256] (128 x 256, row-major),
// b_F (256), b' (128), zeros.
constexpr int C_WFT = 2 * F_TOTAL * 256, C_WFT_END = C_WFT + 256 * 256;
constexpr int C_WD1 = (2 * L::F_TOTAL + 2 * B_PADDED) * 256, C_BF = C_WD1 + 128 * 256, C_BP = C_BF + 256, C_USED = C_BP + 128;
constexpr int C_END = (2 * L::F_TOTAL + 2 * 1104) * 256;                                        // end of the image
static_assert(C_WFT_END == 2 * L::F_TOTAL * 256, "W_F^T fills the forward stream's freed fragments exactly");
static_assert(C_USED <= C_END, "the copies fit the transposed stream's freed fragments");
}  // namespace LF
__host__ __device__ constexpr int fold_wp(int n, int k) { return -2 - (n * 256 + k); }
__host__ __device__ constexpr bool is_fold_wp(int src) { return src <= -2; }
__host__ __device__ constexpr int fold_wp_n(int src) { return (-2 - src) >> 8; }
__host__ __device__ constexpr int fold_wp_k(int src) { return (-2 - src) & 255; }

__host__ __device__ constexpr int fwd_index_fold(int f, int r, int h, int j) {
  if (f < LF::F_A) return fwd_index(f, r, h, j);       // trunk
  if (f < LF::F_DIR) return r == 0 ? L::P_WA + kperm(f - LF::F_A, h, j) : -1;                   // alpha: row 0 of one tile, K = 256
  if (f < LF::F_RGB) {                                 // dir0': [h7(256), dirPE(27+5 pad)] vs [W' | WD[:, 256:]]
    const int g = f - LF::F_DIR;
    const int nt = g / 18, ks = g % 18;
    const int kk = kperm(ks, h, j), n = 32 * nt + r;
    if (kk < 256) return fold_wp(n, kk);
    return (kk - 256) < 27 ? L::P_WD + n * 283 + kk : -1;
  }
  const int ks = f - LF::F_RGB;                        // rgb
  return r < 3 ? L::P_WR + r * 128 + kperm(ks, h, j) : -1;
}
__host__ __device__ constexpr int bwd_index_fold(int f, int r, int h, int j) {
  if (f < LF::B_DA) return bwd_index(f, r, h, j);      // rgb^T
  if (f < LF::B_L7) {                                  // [W'; alpha]^T: 8 tiles of h7 x 9 k-steps (dZ_D 0..127, d alpha 128)
    const int g = f - LF::B_DA, kt = g / 9, ns = g % 9;
    const int nn = kperm(ns, h, j), row = 32 * kt + r;
    if (ns < 8) return fold_wp(nn, row);
    return nn == 128 ? L::P_WA + row : -1;
  }
  return bwd_index(f + LF::B_SHIFT, r, h, j);          // pos7 .. pos1
}

// bias slot s -> offset of the master parameter, -1 = zero padding
__host__ __device__ constexpr int bias_index(int s) {
  if (s < L::BI_FEAT) return L::pb(s >> 8) + (s & 255);
  if (s < L::BI_ALPHA) return L::P_BF + (s - L::BI_FEAT);
  if (s < L::BI_DIR) return s == L::BI_ALPHA ? L::P_BA : -1;
  if (s < L::BI_RGB) return L::P_BD + (s - L::BI_DIR);
  return (s - L::BI_RGB) < 3 ? L::P_BR + (s - L::BI_RGB) : -1;
}
// What the pack routine (mlp_pack.h) needs to know of a model: fragment counts of its two streams, used and padded, its bias
// slots, and the three maps.  (out_ch: the image model's; unused here)
struct ViewPack {
  static constexpr int F_TOTAL = L::F_TOTAL, F_PADDED = L::F_TOTAL, B_TOTAL = L::B_TOTAL, B_PADDED = L::B_PADDED, BI_TOTAL = L::BI_TOTAL;
  static __host__ __device__ constexpr int fwd(int f, int r, int h, int j, int) { return fwd_index(f, r, h, j); }
  static __host__ __device__ constexpr int bwd(int f, int r, int h, int j, int) { return bwd_index(f, r, h, j); }
  static __host__ __device__ constexpr int bias(int s, int) { return bias_index(s); }
};
// element j of lane (r, h) of fragment f of S's padded forward (fw) or transposed stream: fragments behind the last used one are zero
template <class S>
__host__ __device__ constexpr int pack_index(bool fw, int f, int r, int h, int j, int out_ch) {
  if (f >= (fw ? S::F_TOTAL : S::B_TOTAL)) return -1;
  return fw ? S::fwd(f, r, h, j, out_ch) : S::bwd(f, r, h, j, out_ch);
}

// ------------------------------------------------------------------------------------------
// ... and back, for the two matrices the factored weight gradients read out of the forward stream
// ------------------------------------------------------------------------------------------
struct FragElem { int f, r, h, j; };                   // fragment, lane (r, h), element
// W_F[row][col] (feature layer, 256 x 256): fwd_index(fwd_elem_feature(row, col)) == P_WF + row * 256 + col
__host__ __device__ constexpr FragElem fwd_elem_feature(int row, int col) {
  return FragElem{L::F_FA + 16 * (row >> 5) + kperm_ks(col), row & 31, kperm_h(col), kperm_j(col)};
}
// W_D[row][col], col < 256 (dir0 layer, feature columns): fwd_index(fwd_elem_dir0(row, col)) == P_WD + row * 283 + col
__host__ __device__ constexpr FragElem fwd_elem_dir0(int row, int col) {
  return FragElem{L::F_DIR + 18 * (row >> 5) + kperm_ks(col), row & 31, kperm_h(col), kperm_j(col)};
}
// W'[n][k] in the folded streams: fwd_index_fold(fold_elem_fwd(n, k)) == bwd_index_fold(fold_elem_bwd(n, k)) == fold_wp(n, k)
__host__ __device__ constexpr FragElem fold_elem_fwd(int n, int k) {
  return FragElem{LF::F_DIR + 18 * (n >> 5) + kperm_ks(k), n & 31, kperm_h(k), kperm_j(k)};
}
__host__ __device__ constexpr FragElem fold_elem_bwd(int n, int k) {
  return FragElem{LF::B_DA + 9 * (k >> 5) + kperm_ks(n), k & 31, kperm_h(n), kperm_j(n)};
}
// bf16 element index of a fragment element in a weight stream of 1 KiB fragments: lane 32 h + r holds eight elements of 2 bytes
__host__ __device__ constexpr int frag_elem_offset(const FragElem& e) { return (e.f * 64 + 32 * e.h + e.r) * 8 + e.j; }

}  // namespace nerf
