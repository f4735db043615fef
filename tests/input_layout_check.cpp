// Stand-alone check of csrc/mlp_input.h (host compiler, -fsanitize=address,undefined; run by tests/test_input_layout_host.py): the
// channel order of the view model's input stage.  Both encoders (channel pairs, lane groups) and both embedded-row readers are
// instantiated with a host evaluator -- sin / cos in double of the float32 product x * f -- and a packer that keeps the eight floats,
// and every element they produce must equal, bit for bit, the embedding written out directly in the reference's order
// [x, sin(f0 x), cos(f0 x), ...] (63 channels of a position, 27 of a direction) at the place the maps of csrc/mlp_index.h name:
// kperm for every (k-step, lane half, element) of the pair layout, pos_chan16 / dir_chan16 for every (k-step, lane group, element)
// of the group layout; pad elements must be +0.  Both frequency modes of fill_freqs, three points.
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../nerf_meets_mlx_amd/csrc/mlp_index.h"
#include "../nerf_meets_mlx_amd/csrc/mlp_input.h"

using namespace nerf;

struct HostSin : ByPhase<HostSin> {
  static float sin_ph(float x, float f, float ph) {
    const float a = x * f;
    return (float)(ph != 0.0f ? cos((double)a) : sin((double)a));
  }
};
struct Keep {
  static void pack(const float (&v)[8], float (&o)[8]) { memcpy(o, v, sizeof o); }
};

// models/embedding.py:30-71
static std::vector<float> embed(const float (&x)[3], const float* freqs, int nb) {
  std::vector<float> e(x, x + 3);
  for (int k = 0; k < nb; ++k) {
    for (int d = 0; d < 3; ++d) { const float a = x[d] * freqs[k]; e.push_back((float)sin((double)a)); }
    for (int d = 0; d < 3; ++d) { const float a = x[d] * freqs[k]; e.push_back((float)cos((double)a)); }
  }
  return e;
}

static long long checked = 0;
static int bad = 0;
static void expect(float got, float want, const char* what, int a, int b, int c) {
  ++checked;
  if (memcmp(&got, &want, 4) != 0 && bad++ < 10) fprintf(stderr, "MISMATCH %s at (%d, %d, %d): got %.9g, want %.9g\n", what, a, b, c, got, want);
}
static float at(const std::vector<float>& e, int c) { return c >= 0 && c < (int)e.size() ? e[(size_t)c] : 0.0f; }

template <int KS, int LIMIT, int NB>
static void check_pairs(const float (&x)[3], const float (&fr)[NB], const std::vector<float>& e, const char* what) {
  for (int h = 0; h < 2; ++h) {
    float enc[8], row[8];
    encode_pairs<HostSin, Keep, KS, LIMIT, NB>(x, fr, h, enc);
    row_pairs<Keep>(e.data(), KS, h, LIMIT, row);
    for (int j = 0; j < 8; ++j) {
      expect(enc[j], at(e, kperm(KS, h, j)), what, KS, h, j);
      expect(row[j], at(e, kperm(KS, h, j)), "row of the pair layout", KS, h, j);
    }
  }
}

int main() {
  const float pts[3][2][3] = {{{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}},
                              {{-1.25f, 0.5f, 3.0f}, {-0.6f, 0.64f, 0.48f}},
                              {{3.5f, -4.0f, 2.9f}, {0.267f, -0.535f, 0.802f}}};      // |p| = 6.06: the far end of the argument range
  for (int mode = 0; mode < 2; ++mode) {
    PeFreq fr;
    fill_freqs(fr.pos, fr.dir, mode);
    for (const auto& pt : pts) {
      const float (&p)[3] = pt[0];
      const float (&d)[3] = pt[1];
      const std::vector<float> ep = embed(p, fr.pos, 10), ed = embed(d, fr.dir, 4);
      if (ep.size() != 63 || ed.size() != 27) { fprintf(stderr, "embedding sizes\n"); return 2; }
      // channel pairs: 4 + 2 k-steps of 16 channels
      check_pairs<0, 63, 10>(p, fr.pos, ep, "position pairs"); check_pairs<1, 63, 10>(p, fr.pos, ep, "position pairs");
      check_pairs<2, 63, 10>(p, fr.pos, ep, "position pairs"); check_pairs<3, 63, 10>(p, fr.pos, ep, "position pairs");
      check_pairs<0, 27, 4>(d, fr.dir, ed, "direction pairs"); check_pairs<1, 27, 4>(d, fr.dir, ed, "direction pairs");
      // lane groups: 2 + 1 k-steps of 32 channels
      for (int g = 0; g < 4; ++g) {
        const GroupFreq q = group_freqs(fr, g);
        float enc[2][8], row[2][8], denc[1][8], drow[1][8];
        encode_group<HostSin, Keep, false>(q, p, enc);
        encode_group<HostSin, Keep, true>(q, d, denc);
        row_group<Keep, false>(ep.data(), g, row);
        row_group<Keep, true>(ed.data(), g, drow);
        for (int j = 0; j < 8; ++j) {
          for (int ks = 0; ks < 2; ++ks) {
            expect(enc[ks][j], at(ep, pos_chan16(ks, g, j)), "position groups", ks, g, j);
            expect(row[ks][j], at(ep, pos_chan16(ks, g, j)), "position row of the group layout", ks, g, j);
          }
          expect(denc[0][j], at(ed, dir_chan16(g, j)), "direction groups", 0, g, j);
          expect(drow[0][j], at(ed, dir_chan16(g, j)), "direction row of the group layout", 0, g, j);
        }
      }
    }
  }
  // the maps place every channel exactly once
  std::vector<int> seen(63 + 27, 0);
  for (int g = 0; g < 4; ++g)
    for (int j = 0; j < 8; ++j) {
      for (int ks = 0; ks < 2; ++ks) { const int c = pos_chan16(ks, g, j); if (c >= 63) ++bad; else if (c >= 0) ++seen[(size_t)c]; }
      const int c = dir_chan16(g, j);
      if (c >= 27) ++bad; else if (c >= 0) ++seen[(size_t)(63 + c)];
    }
  for (int c : seen) if (c != 1) ++bad;
  printf("input_layout_check: %lld elements, %d bad\n", checked, bad);
  return bad ? 1 : 0;
}
