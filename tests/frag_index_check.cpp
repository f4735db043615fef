// Stand-alone check of csrc/mlp_index.h (host compiler, -fsanitize=address,undefined; run by tests/test_frag_index_host.py):
// the post step of the factored weight gradients (csrc/mlp_dwf.hip) reads W_F and W_D[:, :256] out of the packed forward stream
// through fwd_elem_feature / fwd_elem_dir0.  For every (row, column) of the two matrices the element they name must be the one the
// packing's forward map fwd_index fills with exactly that parameter; every fragment element that fwd_index fills with a parameter of
// the two matrices must be named exactly once (none missed, none twice), and kperm_ks / kperm_h / kperm_j must invert kperm.
#include <stdio.h>
#include <vector>
#include "../nerf_meets_mlx_amd/csrc/mlp_index.h"

using namespace nerf;

int main() {
  int bad = 0;
  auto fail = [&](const char* what, int a, int b) { if (bad++ < 10) fprintf(stderr, "MISMATCH %s at (%d, %d)\n", what, a, b); };
  // kperm and its inverse: a bijection of [0, 16) per k-step
  for (int ks = 0; ks < 18; ++ks) {
    std::vector<int> seen(16, 0);
    for (int h = 0; h < 2; ++h)
      for (int j = 0; j < 8; ++j) {
        const int kk = kperm(ks, h, j);
        if (kk < 16 * ks || kk >= 16 * ks + 16) { fail("kperm range", ks, 8 * h + j); continue; }
        ++seen[kk - 16 * ks];
        if (kperm_ks(kk) != ks || kperm_h(kk) != h || kperm_j(kk) != j) fail("kperm inverse", ks, 8 * h + j);
      }
    for (int c = 0; c < 16; ++c) if (seen[c] != 1) fail("kperm cover", ks, c);
  }
  // hits[element of the forward stream] = how often the inverse maps name it
  std::vector<int> hits((size_t)L::F_TOTAL * 512, 0);
  auto visit = [&](const FragElem& e, int want, int row, int col, const char* what) {
    if (e.f < 0 || e.f >= L::F_TOTAL || e.r < 0 || e.r >= 32 || e.h < 0 || e.h >= 2 || e.j < 0 || e.j >= 8) { fail(what, row, col); return; }
    if (fwd_index(e.f, e.r, e.h, e.j) != want) fail(what, row, col);
    const int off = frag_elem_offset(e);
    if (off != ((e.f * 64 + 32 * e.h + e.r) * 8 + e.j)) fail("offset", row, col);
    ++hits[(size_t)off];
  };
  long long walked = 0;
  for (int row = 0; row < 256; ++row)
    for (int col = 0; col < 256; ++col, ++walked) visit(fwd_elem_feature(row, col), L::P_WF + row * 256 + col, row, col, "W_F");
  for (int row = 0; row < 128; ++row)
    for (int col = 0; col < 256; ++col, ++walked) visit(fwd_elem_dir0(row, col), L::P_WD + row * 283 + col, row, col, "W_D");
  // the other direction: every element the packing fills with a parameter of W_F or W_D[:, :256] was named once, every other never
  long long filled = 0;
  for (int f = 0; f < L::F_TOTAL; ++f)
    for (int h = 0; h < 2; ++h)
      for (int r = 0; r < 32; ++r)
        for (int j = 0; j < 8; ++j) {
          const int p = fwd_index(f, r, h, j);
          const bool in_f = p >= L::P_WF && p < L::P_WF + 256 * 256;
          const bool in_d = p >= L::P_WD && p < L::P_WD + 128 * 283 && (p - L::P_WD) % 283 < 256;
          const int n = hits[(size_t)frag_elem_offset(FragElem{f, r, h, j})];
          if (n != ((in_f || in_d) ? 1 : 0)) fail("cover", f, 64 * h + 2 * r);
          filled += (in_f || in_d) ? 1 : 0;
        }
  if (filled != walked || walked != 256 * 256 + 128 * 256) fail("count", (int)filled, (int)walked);
  printf("frag_index_check: %lld elements, %d bad\n", walked, bad);
  return bad ? 1 : 0;
}
