// Stand-alone check of the packing maps of all three model shapes and of the 2 x 64 model's input stage (host compiler,
// -fsanitize=address,undefined; run by tests/test_pack_index_host.py).  csrc/mlp_pack.h fills the weight streams through
// ViewPack (csrc/mlp_index.h), ImgPack and SmallPack (csrc/mlp_arch2.h):
//   forward streams   every weight of the model is named exactly once, no bias ever, the rest is padding;
//   backward streams  nothing is named twice, no bias ever, and the weights never named are exactly the columns whose input takes
//                     no gradient (image: W0 and the 40 input columns of W5; 2 x 64: the 16 SH columns of W_D; view: W0, the 63
//                     encoding columns of W5, the 27 encoding columns of W_D);
//   bias slots        every bias is named exactly once, no weight ever.
// csrc/mlp_input2.h: the fused row stage's channel map is kperm for all 32 + 16 elements, and small_tile_sample gives every sample
// to exactly one valid lane, in both tile orders, and keeps every other lane's sample inside [0, B n).
#include <stdio.h>
#include <stdint.h>
#include <vector>
#include "../nerf_meets_mlx_amd/csrc/mlp_input2.h"

using namespace nerf;

static int bad = 0;
static void fail(const char* model, const char* what, long long a, long long b) {
  if (bad++ < 20) fprintf(stderr, "MISMATCH %s: %s (%lld, %lld)\n", model, what, a, b);
}

struct Range { int off, rows, ld, col0, cols; };       // parameters off + row * ld + col0 + [0, cols), row < rows

// biases / dead: the parameter ranges that are biases / weights whose input takes no gradient
template <class S>
static void check(const char* name, int out_ch, int params, const std::vector<Range>& biases, const std::vector<Range>& dead,
                  long long want_fwd_once, long long want_fwd_pad, long long want_bwd_once, long long want_bwd_never) {
  std::vector<char> is_bias((size_t)params, 0), is_dead((size_t)params, 0);
  auto mark = [&](std::vector<char>& v, const std::vector<Range>& rs) {
    for (const Range& g : rs)
      for (int row = 0; row < g.rows; ++row)
        for (int c = 0; c < g.cols; ++c) v[(size_t)(g.off + row * g.ld + g.col0 + c)] = 1;
  };
  mark(is_bias, biases);
  mark(is_dead, dead);
  long long nbias = 0;
  for (char b : is_bias) nbias += b;
  for (int fw = 1; fw >= 0; --fw) {
    std::vector<int> hits((size_t)params, 0);
    long long pad = 0;
    for (int f = 0; f < (fw ? S::F_PADDED : S::B_PADDED); ++f)
      for (int h = 0; h < 2; ++h)
        for (int r = 0; r < 32; ++r)
          for (int j = 0; j < 8; ++j) {
            const int p = pack_index<S>(fw != 0, f, r, h, j, out_ch);
            if (p < -1 || p >= params) { fail(name, fw ? "forward offset out of range" : "backward offset out of range", f, p); continue; }
            if (p < 0) ++pad; else ++hits[(size_t)p];
          }
    long long once = 0, never = 0;
    for (int p = 0; p < params; ++p) {
      const int n = hits[(size_t)p];
      once += n == 1; never += n == 0;
      if (n > 1) fail(name, fw ? "named twice in the forward stream" : "named twice in the backward stream", p, n);
      if (is_bias[(size_t)p] && n) fail(name, "a bias in a weight stream", p, fw);
      if (fw && !is_bias[(size_t)p] && n != 1) fail(name, "weight not named once in the forward stream", p, n);
      if (!fw && !is_bias[(size_t)p] && (n == 0) != (is_dead[(size_t)p] != 0)) fail(name, "backward stream: wrong set of unnamed weights", p, n);
    }
    if (fw) {
      if (once != want_fwd_once || never != nbias || pad != want_fwd_pad) fail(name, "forward counts", once, pad);
      printf("%s out_ch %d forward: %lld named once, %lld never, %lld padding\n", name, out_ch, once, never, pad);
    } else {
      if (once != want_bwd_once || never != want_bwd_never) fail(name, "backward counts", once, never);
      printf("%s out_ch %d backward: %lld named once, %lld never\n", name, out_ch, once, never);
    }
  }
  std::vector<int> hits((size_t)params, 0);
  for (int s = 0; s < S::BI_TOTAL; ++s) {
    const int p = S::bias(s, out_ch);
    if (p < -1 || p >= params) { fail(name, "bias offset out of range", s, p); continue; }
    if (p >= 0) ++hits[(size_t)p];
  }
  for (int p = 0; p < params; ++p)
    if (hits[(size_t)p] != (is_bias[(size_t)p] ? 1 : 0)) fail(name, "bias slots", p, hits[(size_t)p]);
}

struct Query { int64_t M, B; int n, ray_major; };

int main() {
  {
    std::vector<Range> b, dead = {{L::P_W0, 256, 63, 0, 63}, {L::P_W5, 256, 319, 0, 63}, {L::P_WD, 128, 283, 256, 27}};
    for (int l = 0; l < 8; ++l) b.push_back({L::pb(l), 1, 0, 0, 256});
    b.push_back({L::P_BF, 1, 0, 0, 256}); b.push_back({L::P_BA, 1, 0, 0, 1}); b.push_back({L::P_BD, 1, 0, 0, 128}); b.push_back({L::P_BR, 1, 0, 0, 3});
    const long long w = L::P_TOTAL - (8 * 256 + 256 + 1 + 128 + 3), d = 256 * 63 * 2 + 128 * 27;
    check<ViewPack>("view", 0, L::P_TOTAL, b, dead, w, (long long)L::F_TOTAL * 512 - w, w - d, L::P_TOTAL - (w - d));
  }
  const long long img_fwd[4] = {479488, 479744, 480000, 480256}, img_pad[4] = {12032, 11776, 11520, 11264};
  const long long img_bwd[4] = {459008, 459264, 459520, 459776};
  for (int oc = 1; oc <= 4; ++oc) {
    std::vector<Range> b, dead = {{LI::P_W0, 256, 40, 0, 40}, {LI::P_W5, 256, 296, 0, 40}};
    for (int l = 0; l < 8; ++l) b.push_back({LI::pb(l), 1, 0, 0, 256});
    b.push_back({LI::P_WO + oc * 256, 1, 0, 0, oc});
    check<ImgPack>("image", oc, LI::P_WO + oc * 257, b, dead, img_fwd[oc - 1], img_pad[oc - 1], img_bwd[oc - 1], 22528 + oc);
  }
  {
    std::vector<Range> b = {{LN::P_B0, 1, 0, 0, 64}, {LN::P_B1, 1, 0, 0, 64}, {LN::P_BF, 1, 0, 0, 64}, {LN::P_BA, 1, 0, 0, 1},
                            {LN::P_BD, 1, 0, 0, 32}, {LN::P_BR, 1, 0, 0, 3}};
    std::vector<Range> dead = {{LN::P_WD, 32, 80, 64, 16}};
    check<SmallPack>("2x64", 0, LN::P_TOTAL, b, dead, 12960, 3424, 12448, 740);
  }
  // fused row stage: element j of lane half h
  int elems = 0;
  for (int h = 0; h < 2; ++h)
    for (int j = 0; j < 8; ++j) {
      for (int ks = 0; ks < 2; ++ks, ++elems) {
        const int c = kperm(ks, h, j);
        if (ngp_pos_level(ks, h, j) != (c >> 1) || (j & 1) != (c & 1)) fail("2x64", "position channel map", ks, 8 * h + j);
      }
      if (ngp_sh_chan(h, j) != kperm(0, h, j)) fail("2x64", "SH channel map", h, j);
      ++elems;
    }
  if (elems != 48) fail("2x64", "channel count", elems, 48);
  // tile map
  const int cases[4][2] = {{1, 1}, {31, 2}, {33, 3}, {64, 1}};
  for (const auto& c : cases)
    for (int rmaj = 0; rmaj < 2; ++rmaj) {
      const Query q{(int64_t)c[0] * c[1], c[0], c[1], rmaj};
      std::vector<int> owners((size_t)q.M, 0);
      const int64_t ntiles = small_tiles(q);
      for (int64_t t = 0; t < ntiles; ++t)
        for (int r = 0; r < 32; ++r) {
          const TileSample ts = small_tile_sample(q, t, r, rmaj != 0);
          if (ts.m < 0 || ts.m >= q.M) { fail("2x64", "tile map: sample out of range", t, r); continue; }
          if (ts.valid) ++owners[(size_t)ts.m];
        }
      for (int64_t m = 0; m < q.M; ++m)
        if (owners[(size_t)m] != 1) fail("2x64", rmaj ? "ray-major tiles: owners of a sample" : "sample-major tiles: owners of a sample", m, owners[(size_t)m]);
    }
  if (small_ray_major(false, 1, 31) || !small_ray_major(false, 1, 32) || small_ray_major(true, 1, 64) || small_ray_major(false, 0, 64))
    fail("2x64", "ray-major rule", 0, 0);
  printf("pack_index_check: %d channel elements, %d bad\n", elems, bad);
  return bad ? 1 : 0;
}
