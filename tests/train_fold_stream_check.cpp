// Stand-alone check of the FOLDED split-bf16 training image's source maps (csrc/mlp_index.h: fwd_index_fold / bwd_index_fold, namespace
// LF; host compiler, -fsanitize=address,undefined; run by tests/test_train_fold_stream_host.py).  Both streams carry
// W' = W_D[:, :256] W_F where the unfolded ones carried W_F and W_D[:, :256]:
//   * forward stream: every weight of pos0..pos7, alpha, W_D[:, 256:283] and rgb is named by exactly one fragment element, W_F, b_F,
//     W_D[:, :256] and the biases by none, and each of the 128 x 256 elements of W' exactly once, at the pair and element the kernel's
//     layer_fwd<18, 4> reads it from (pair F_DIR + 18 nt + ks, row 32 nt + r, input feature kperm(ks, h, j));
//   * transposed stream: the H4 columns of pos5, pos6, pos7, pos1..4, alpha and rgb once each, every element of W' exactly once at the pair
//     layer_bwd<9, 8> reads it from (pair B_DA + 9 kt + ns, row 32 kt + r of h7, dZ_D unit kperm(ns, h, j)); the trunk is the unfolded
//     stream's, 128 pairs earlier;
//   * fold_elem_fwd / fold_elem_bwd invert the two maps;
//   * pair, fragment and ring chunk counts: a ring wraps modulo ceil(fragments / 32) chunks;
//   * the fp32 copies (W_F transposed, W_D[:, :256], b_F, b') lie behind the streamed fragments of their stream, inside the image, and
//     do not overlap one another; the image keeps its size.
#include <stdio.h>
#include <vector>
#include "../nerf_meets_mlx_amd/csrc/mlp_index.h"

using namespace nerf;

// the unfolded image (csrc/mlp_s16.h; repeated here because that header needs the HIP runtime): pair streams of 2 x 1184 and 2 x 1104 fragments
constexpr int S16_F_FRAGS = 2368, S16_B_PADDED = 2208, RING_CHUNK = 32;

int main() {
  int bad = 0;
  auto fail = [&](const char* what, int a, int b) { if (bad++ < 10) fprintf(stderr, "MISMATCH %s at (%d, %d)\n", what, a, b); };
  // counts
  if (LF::F_TOTAL != 1056 || LF::F_TOTAL != L::F_TOTAL - 128 || LF::B_TOTAL != 972 || LF::B_TOTAL != L::B_TOTAL - 128) fail("pairs", LF::F_TOTAL, LF::B_TOTAL);
  if (LF::F_A != 960 || LF::F_DIR != 976 || LF::F_RGB != 1048 || LF::B_DA != 4 || LF::B_L7 != 76) fail("offsets", LF::F_DIR, LF::B_L7);
  const int f_frags = 2 * LF::F_TOTAL, b_frags = 2 * LF::B_TOTAL, b_padded = 2 * LF::B_PADDED;
  const int f_chunks = (f_frags + RING_CHUNK - 1) / RING_CHUNK, b_chunks = (b_frags + RING_CHUNK - 1) / RING_CHUNK;
  if (f_chunks != 66 || f_chunks * RING_CHUNK != f_frags) fail("forward chunks", f_chunks, f_frags);
  if (b_chunks != 61 || b_chunks * RING_CHUNK != b_padded || b_padded < b_frags) fail("transposed chunks", b_chunks, b_padded);
  if (f_frags % 4 || b_frags % 4) fail("fragment groups", f_frags, b_frags);
  // fp32 copies: float ranges of the image (a fragment is 256 floats)
  struct Range { const char* what; long long lo, hi; };
  const Range copies[] = {{"W_F^T", LF::C_WFT, LF::C_WFT_END}, {"W_D1", LF::C_WD1, LF::C_BF}, {"b_F", LF::C_BF, LF::C_BP}, {"b'", LF::C_BP, LF::C_USED}};
  const Range streams[] = {{"forward stream", 0, (long long)f_frags * 256}, {"transposed stream", (long long)S16_F_FRAGS * 256, (long long)(S16_F_FRAGS + b_padded) * 256}};
  if (LF::C_END != (S16_F_FRAGS + S16_B_PADDED) * 256) fail("image size", LF::C_END, 0);
  if (LF::C_WFT_END - LF::C_WFT != 256 * 256 || LF::C_BF - LF::C_WD1 != 128 * 256 || LF::C_BP - LF::C_BF != 256 || LF::C_USED - LF::C_BP != 128) fail("copy sizes", 0, 0);
  for (int a = 0; a < 4; ++a) {
    if (copies[a].lo < 0 || copies[a].hi > LF::C_END || copies[a].lo >= copies[a].hi) fail("copy outside the image", a, 0);
    for (int s = 0; s < 2; ++s) if (copies[a].lo < streams[s].hi && streams[s].lo < copies[a].hi) fail("copy overlaps a stream", a, s);
    for (int b = a + 1; b < 4; ++b) if (copies[a].lo < copies[b].hi && copies[b].lo < copies[a].hi) fail("copies overlap", a, b);
  }
  if (copies[0].hi > streams[1].lo) fail("W_F^T runs into the transposed stream", 0, 0);

  // ---- forward stream
  std::vector<int> hits((size_t)L::P_TOTAL, 0), fold_hits(128 * 256, 0);
  long long fold_named = 0, params_named = 0;
  for (int f = 0; f < LF::F_TOTAL; ++f)
    for (int r = 0; r < 32; ++r)
      for (int h = 0; h < 2; ++h)
        for (int j = 0; j < 8; ++j) {
          const int s = fwd_index_fold(f, r, h, j);
          if (s >= 0) {
            if (s >= L::P_TOTAL) { fail("parameter range", f, s); continue; }
            ++hits[(size_t)s]; ++params_named;
            if (f < LF::F_A && s != fwd_index(f, r, h, j)) fail("trunk differs from the unfolded stream", f, j);
          } else if (is_fold_wp(s)) {
            const int g = f - LF::F_DIR, nt = g / 18, ks = g % 18;
            const int n = fold_wp_n(s), k = fold_wp_k(s);
            if (f < LF::F_DIR || f >= LF::F_RGB || ks >= 16) { fail("W' outside dir0'", f, j); continue; }
            if (n != 32 * nt + r || k != kperm(ks, h, j) || n >= 128 || k >= 256 || fold_wp(n, k) != s) { fail("W' position", f, 8 * (32 * h + r) + j); continue; }
            const FragElem e = fold_elem_fwd(n, k);
            if (e.f != f || e.r != r || e.h != h || e.j != j) fail("fold_elem_fwd", n, k);
            ++fold_hits[(size_t)n * 256 + k]; ++fold_named;
          } else if (s != -1) fail("source kind", f, s);
        }
  for (int e = 0; e < 128 * 256; ++e) if (fold_hits[e] != 1) fail("W' cover (forward)", e / 256, e % 256);
  std::vector<int> want((size_t)L::P_TOTAL, 0);
  long long expected = 0;
  auto mark = [&](int off, int rows, int cols, int stride, int col0) {
    for (int r = 0; r < rows; ++r) for (int c = 0; c < cols; ++c) { want[(size_t)off + r * stride + col0 + c] = 1; ++expected; }
  };
  for (int l = 0; l < 8; ++l) mark(L::pw(l), 256, L::pin(l), L::pin(l), 0);
  mark(L::P_WA, 1, 256, 256, 0);
  mark(L::P_WD, 128, 27, 283, 256);
  mark(L::P_WR, 3, 128, 128, 0);
  for (int p = 0; p < L::P_TOTAL; ++p) if (hits[p] != want[p]) fail("parameter cover (forward)", p, hits[p]);
  if (params_named != expected) fail("parameter count (forward)", (int)params_named, (int)expected);
  for (int p = L::P_WF; p < L::P_WA; ++p) if (hits[p]) fail("forward reads W_F / b_F", p, 0);
  for (int n = 0; n < 128; ++n) for (int c = 0; c < 256; ++c) if (hits[L::P_WD + n * 283 + c]) fail("forward reads W_D[:, :256]", n, c);
  // the heads and dir0's direction columns where the kernel reads them
  for (int ks = 0; ks < 16; ++ks) for (int h = 0; h < 2; ++h) for (int j = 0; j < 8; ++j)
    if (fwd_index_fold(LF::F_A + ks, 0, h, j) != L::P_WA + kperm(ks, h, j)) fail("alpha head", ks, 8 * h + j);
  for (int ks = 0; ks < 8; ++ks) for (int i = 0; i < 3; ++i) for (int h = 0; h < 2; ++h) for (int j = 0; j < 8; ++j)
    if (fwd_index_fold(LF::F_RGB + ks, i, h, j) != L::P_WR + i * 128 + kperm(ks, h, j)) fail("rgb head", ks, 8 * h + j);
  for (int nt = 0; nt < 4; ++nt) for (int ks = 16; ks < 18; ++ks) for (int r = 0; r < 32; ++r) for (int h = 0; h < 2; ++h) for (int j = 0; j < 8; ++j) {
    const int kk = kperm(ks, h, j);
    if (fwd_index_fold(LF::F_DIR + 18 * nt + ks, r, h, j) != (kk < 283 ? L::P_WD + (32 * nt + r) * 283 + kk : -1)) fail("dir0 direction columns", nt, ks);
  }

  // ---- transposed stream
  std::vector<int> bhits((size_t)L::P_TOTAL, 0), bwant((size_t)L::P_TOTAL, 0), bfold(128 * 256, 0);
  long long bfold_named = 0, bparams = 0, bexpected = 0;
  for (int f = 0; f < LF::B_TOTAL; ++f)
    for (int r = 0; r < 32; ++r)
      for (int h = 0; h < 2; ++h)
        for (int j = 0; j < 8; ++j) {
          const int s = bwd_index_fold(f, r, h, j);
          if (s >= 0) {
            if (s >= L::P_TOTAL) { fail("parameter range (transposed)", f, s); continue; }
            ++bhits[(size_t)s]; ++bparams;
            if (f >= LF::B_L7 && s != bwd_index(f + LF::B_SHIFT, r, h, j)) fail("trunk differs from the unfolded stream (transposed)", f, j);
          } else if (is_fold_wp(s)) {
            const int g = f - LF::B_DA, kt = g / 9, ns = g % 9;
            const int n = fold_wp_n(s), k = fold_wp_k(s);
            if (f < LF::B_DA || f >= LF::B_L7 || ns >= 8) { fail("W' outside [W'; alpha]^T", f, j); continue; }
            if (k != 32 * kt + r || n != kperm(ns, h, j) || n >= 128 || k >= 256) { fail("W' position (transposed)", f, 8 * (32 * h + r) + j); continue; }
            const FragElem e = fold_elem_bwd(n, k);
            if (e.f != f || e.r != r || e.h != h || e.j != j) fail("fold_elem_bwd", n, k);
            ++bfold[(size_t)n * 256 + k]; ++bfold_named;
          } else if (s != -1) fail("source kind (transposed)", f, s);
        }
  for (int e = 0; e < 128 * 256; ++e) if (bfold[e] != 1) fail("W' cover (transposed)", e / 256, e % 256);
  auto bmark = [&](int off, int rows, int cols, int stride, int col0) {
    for (int r = 0; r < rows; ++r) for (int c = 0; c < cols; ++c) { bwant[(size_t)off + r * stride + col0 + c] = 1; ++bexpected; }
  };
  for (int l = 1; l < 8; ++l) bmark(L::pw(l), 256, 256, L::pin(l), l == 5 ? 63 : 0);      // pos0 has no input gradient; pos5: its H4 columns
  bmark(L::P_WA, 1, 256, 256, 0);
  bmark(L::P_WR, 3, 128, 128, 0);
  for (int p = 0; p < L::P_TOTAL; ++p) if (bhits[p] != bwant[p]) fail("parameter cover (transposed)", p, bhits[p]);
  if (bparams != bexpected) fail("parameter count (transposed)", (int)bparams, (int)bexpected);
  // d alpha is row kperm(8, 0, 0) == 128 of the ninth k-step
  for (int kt = 0; kt < 8; ++kt) for (int r = 0; r < 32; ++r) for (int h = 0; h < 2; ++h) for (int j = 0; j < 8; ++j)
    if (bwd_index_fold(LF::B_DA + 9 * kt + 8, r, h, j) != (kperm(8, h, j) == 128 ? L::P_WA + 32 * kt + r : -1)) fail("alpha column", kt, r);

  printf("train_fold_stream_check: %d + %d pairs, %d + %d chunks, %lld + %lld parameters, %lld + %lld folded elements, %d bad\n", LF::F_TOTAL,
         LF::B_TOTAL, f_chunks, b_chunks, params_named, bparams, fold_named, bfold_named, bad);
  return bad ? 1 : 0;
}
