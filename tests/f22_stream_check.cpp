// Stand-alone check of the folded split-fp16 forward stream's source map (csrc/mlp22.h, stream_src; host compiler,
// -fsanitize=address,undefined; run by tests/test_f22_stream_host.py).  The stream carries W' = W_D[:, :256] W_F where the unfolded one
// carried W_F and W_D[:, :256]:
//   * every weight of pos0..pos7, alpha, W_D[:, 256:283] and rgb is named by exactly one fragment element, no bias by any;
//   * no element reads W_F, b_F or W_D[:, :256] directly;
//   * the 128 x 256 elements of W' are each named exactly once, in the pair (n-tile, k-step) and at the element the kernel's k-steps
//     expect: layer22's epilogue leaves feature 16 nt + 4 g + i of an output tile nt in lane group g, register 2 (nt & 1) + (i >> 1),
//     half i & 1 of the k-step nt >> 1 -- i.e. element j of lane group g in k-step ks is feature 32 ks + 16 (j >> 2) + 4 g + (j & 3);
//   * every hidden-layer weight sits at the pair pbase + nt KS + ks the kernel reads it from;
//   * pair, fragment and ring chunk counts are the ones mlp22.h states, and the packed image keeps its size.
#include <stdio.h>
#include <vector>
#include "../nerf_meets_mlx_amd/csrc/mlp22.h"

using namespace nerf;
using namespace nerf::f22;

static int expect_k(int ks, int g, int j) { return 32 * ks + 16 * (j >> 2) + 4 * g + (j & 3); }

int main() {
  static_assert(NERF_F22_FOLD == 1, "the shipped form is the folded stream");
  int bad = 0;
  auto fail = [&](const char* what, int a, int b) { if (bad++ < 10) fprintf(stderr, "MISMATCH %s at (%d, %d)\n", what, a, b); };
  // counts
  if (F_PAIRS != 960 + 8 + 72 + 4 || F_PAIRS != 1044 || F_FRAGS != 2088 || F_STREAM != 2112 || CHUNKS != 66) fail("counts", F_PAIRS, CHUNKS);
  if (CHUNKS != (F_FRAGS + 31) / 32 || F_FRAGS % 32 != 8 || F_FRAGS % 4 != 0) fail("chunks", F_FRAGS, CHUNKS);
  if (F_PADDED != 2368 || F_STREAM > F_PADDED || BIAS_FLOATS != 2496 || PACKED_BYTES != 2368 * 1024 + 2496 * 4) fail("image size", F_PADDED, BIAS_FLOATS);
  if (P_ALPHA != 960 || P_DIR != 968 || P_RGB != 1040) fail("offsets", P_DIR, P_RGB);

  std::vector<int> hits((size_t)L::P_TOTAL, 0), fold_hits(128 * 256, 0);
  long long fold_named = 0, params_named = 0;
  for (int fp = 0; fp < F_PADDED / 2; ++fp)
    for (int i = 0; i < 16; ++i)
      for (int g = 0; g < 4; ++g)
        for (int j = 0; j < 8; ++j) {
          const Src s = stream_src(fp, i, g, j);
          if (fp >= F_PAIRS) { if (s.p != SRC_ZERO) fail("padding", fp, 16 * g + i); continue; }
          if (s.p >= 0) {
            if (s.p >= L::P_TOTAL) { fail("parameter range", fp, s.p); continue; }
            ++hits[(size_t)s.p]; ++params_named;
          } else if (s.p == SRC_FOLD) {
            const int q = fp - P_DIR, nt = q / 9, ks = q % 9;
            if (fp < P_DIR || fp >= P_RGB || ks >= 8) { fail("W' outside dir0'", fp, j); continue; }
            if (s.n != 16 * nt + i || s.k != expect_k(ks, g, j) || s.n < 0 || s.n >= 128 || s.k < 0 || s.k >= 256) { fail("W' position", fp, 8 * (16 * g + i) + j); continue; }
            ++fold_hits[(size_t)s.n * 256 + s.k]; ++fold_named;
          } else if (s.p != SRC_ZERO) fail("source kind", fp, s.p);
        }
  for (int e = 0; e < 128 * 256; ++e) if (fold_hits[e] != 1) fail("W' cover", e / 256, e % 256);
  if (fold_named != 128 * 256) fail("W' count", (int)fold_named, 0);

  // expected coverage of the master parameters
  std::vector<int> want((size_t)L::P_TOTAL, 0);
  long long expected = 0;
  auto mark = [&](int off, int rows, int cols, int stride, int col0) {
    for (int r = 0; r < rows; ++r) for (int c = 0; c < cols; ++c) { want[(size_t)off + r * stride + col0 + c] = 1; ++expected; }
  };
  for (int l = 0; l < 8; ++l) mark(L::pw(l), 256, L::pin(l), L::pin(l), 0);
  mark(L::P_WA, 1, 256, 256, 0);
  mark(L::P_WD, 128, 27, 283, 256);
  mark(L::P_WR, 3, 128, 128, 0);
  for (int p = 0; p < L::P_TOTAL; ++p) if (hits[p] != want[p]) fail("parameter cover", p, hits[p]);
  if (params_named != expected) fail("parameter count", (int)params_named, (int)expected);
  // (spelled out: nothing of the folded matrices or their bias, and no bias at all, is read into a fragment)
  for (int p = L::P_WF; p < L::P_WA; ++p) if (hits[p]) fail("reads W_F / b_F", p, 0);
  for (int n = 0; n < 128; ++n) for (int c = 0; c < 256; ++c) if (hits[L::P_WD + n * 283 + c]) fail("reads W_D[:, :256]", n, c);
  for (int p = L::P_BD; p < L::P_WR; ++p) if (hits[p]) fail("reads b_D", p, 0);

  // the hidden layers at the pairs and elements the kernel reads them from: pair pbase + nt KS + ks, row 16 nt + i, input feature expect_k
  struct Layer { int pbase, ks0, KS, w, in, skip; };
  const Layer layers[] = {{P_L1, 0, 8, L::pw(1), 256, 0}, {P_L1 + 128, 0, 8, L::pw(2), 256, 0}, {P_L1 + 256, 0, 8, L::pw(3), 256, 0},
                          {P_L1 + 384, 0, 8, L::pw(4), 256, 0}, {P_L5, 2, 10, L::P_W5, 319, 63}, {P_L6, 0, 8, L::P_W6, 256, 0},
                          {P_L7, 0, 8, L::P_W7, 256, 0}};
  for (const Layer& y : layers)
    for (int nt = 0; nt < 16; ++nt)
      for (int ks = y.ks0; ks < y.KS; ++ks)
        for (int i = 0; i < 16; ++i)
          for (int g = 0; g < 4; ++g)
            for (int j = 0; j < 8; ++j)
              if (stream_src(y.pbase + nt * y.KS + ks, i, g, j).p != y.w + (16 * nt + i) * y.in + y.skip + expect_k(ks - y.ks0, g, j)) fail("hidden layer", y.pbase, nt * y.KS + ks);
  for (int ks = 0; ks < 8; ++ks) for (int g = 0; g < 4; ++g) for (int j = 0; j < 8; ++j) {
    if (stream_src(P_ALPHA + ks, 0, g, j).p != L::P_WA + expect_k(ks, g, j)) fail("alpha head", ks, 8 * g + j);
    if (ks < 4) for (int i = 0; i < 3; ++i) if (stream_src(P_RGB + ks, i, g, j).p != L::P_WR + i * 128 + expect_k(ks, g, j)) fail("rgb head", ks, 8 * g + j);
  }
  printf("f22_stream_check: %d pairs, %d chunks, %lld parameters, %lld folded elements, %d bad\n", F_PAIRS, CHUNKS, params_named, fold_named, bad);
  return bad ? 1 : 0;
}
