// Stand-alone check of csrc/dw_split.h (host compiler, -fsanitize=address,undefined; run by tests/test_mlp_model_host.py):
// every case of tests/golden/dw_split_parent.txt -- the three models' full, wide-only and narrow-only job lists x target workgroups
// x sample tiles x bias, recorded from the loop that lived in launch_dw_part before it became a function -- must give the same
// splits, each within [1, (ntiles + 3) / 4], and a total of at most max(target, jobs).
//   usage: dw_split_check <table>      (format: the table's own header)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../nerf_meets_mlx_amd/csrc/dw_split.h"

static std::vector<long long> numbers(const char* s) {      // every integer of s, in order
  std::vector<long long> v;
  for (char* end; *s; s = end) {
    const long long x = strtoll(s, &end, 10);
    if (end == s) { end = const_cast<char*>(s) + 1; continue; }
    v.push_back(x);
  }
  return v;
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s <table>\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { perror(argv[1]); return 2; }
  constexpr int MAXJ = nerf::DW_SPLIT_MAX_JOBS;
  char line[4096];
  std::vector<long long> tiles, want;
  nerf::DwCost jobs[MAXJ];
  int nj = 0, cases = 0, bad = 0;
  while (fgets(line, sizeof line, f)) {
    if (line[0] == 'N') tiles = numbers(line + 1);
    if (line[0] == 'J') {
      const std::vector<long long> v = numbers(line + 1);
      nj = (int)v.size() / 2;
      if (nj < 1 || nj > MAXJ || v.size() % 2) { fprintf(stderr, "malformed line: %s", line); return 2; }
      for (int j = 0; j < nj; ++j) jobs[j] = nerf::DwCost{(int)v[2 * j], (int)v[2 * j + 1]};
    }
    if (line[0] != 'C') continue;
    char* colon = strchr(line, ':');
    const std::vector<long long> head = numbers(line + 1);       // bias, target, then the entries' numbers
    if (!colon || head.size() < 2 || nj == 0 || tiles.empty()) { fprintf(stderr, "malformed line: %s", line); return 2; }
    const int bias = (int)head[0], target = (int)head[1];
    size_t k = 0;
    for (char* entry = strtok(colon + 1, ";"); entry; entry = strtok(nullptr, ";"), ++k) {
      if (!strchr(entry, '=')) want = numbers(entry);            // '=': the entry before it again
      if (k >= tiles.size() || (int)want.size() != nj + 1) { fprintf(stderr, "malformed entry %zu: %s", k, line); return 2; }
      const long long max_splits = (tiles[k] + 3) / 4;
      int got[MAXJ], sum = 0;
      const int total = nerf::dw_split(jobs, nj, bias, target, max_splits, got);
      bool good = total == want[nj] && total <= (target > nj ? target : nj);
      for (int j = 0; j < MAXJ; ++j) {
        if (j < nj) { good = good && got[j] == want[j] && got[j] >= 1 && got[j] <= max_splits; sum += got[j]; }
        else good = good && got[j] == 0;
      }
      good = good && sum == total;
      if (!good && bad++ < 10) fprintf(stderr, "MISMATCH: %d jobs, bias %d, target %d, %lld tiles: total %d\n", nj, bias, target, tiles[k], total);
      ++cases;
    }
    if (k != tiles.size()) { fprintf(stderr, "%zu entries for %zu tile counts: %s", k, tiles.size(), line); return 2; }
  }
  fclose(f);
  printf("dw_split_check: %d cases, %d bad\n", cases, bad);
  return bad || cases < 1000 ? 1 : 0;
}
