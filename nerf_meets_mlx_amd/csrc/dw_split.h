// How the workgroups of one weight-gradient (dW) launch are shared out over its jobs.  Pure host arithmetic without a HIP
// dependency: the split decides the summation order of every gradient, so it is a function that a CPU test can call
// (tests/dw_split_check.cpp).
#pragma once
#include <stdint.h>

namespace nerf {

constexpr int DW_SPLIT_MAX_JOBS = 16;        // = DW_MAX_JOBS (mlp_frag.h)
struct DwCost { int nf, kf; };               // dZ / input-activation fragments of a job: its bytes per sample tile, in KiB

// splits[j] = workgroups of job j (entries from nj on are zeroed); returns their sum.
//   bias        per-tile fixed cost of a job in fragment units ("dw_unit_bias" or its automatic value)
//   target_wgs  workgroups to hand out: one per CU ("dw_workgroups" overrides), at most the launch's partial-tile slots
//   max_splits  most workgroups per job: (sample tiles + 3) / 4, i.e. >= 4 sample tiles per workgroup
inline int dw_split(const DwCost* jobs, int nj, int bias, int target_wgs, int64_t max_splits, int* splits) {
  // A job's cost per sample tile = its bytes (nf + kf KiB) + a fixed part (barrier, waits, the 4 DMA issues per wave,
  // transposed reads, MFMAs) worth about 128 KiB of streaming: single-job timings fit t = a (nf + kf + c0) with c0 = 24
  // at a full grid, but under load the sweep over c0 keeps improving up to ~128 and is flat beyond (tools/sweep_dw.py).  Split the sample range of every job in proportion.
  // Split-bf16 kernels (round 6): since the 256 x 256 jobs run in a launch of their own (all equal: the bias is moot there), the bias only
  // balances the six narrow jobs among themselves, and their times alone fit t = 9.0 (nf + kf) + 0 ... 14: 32 gave the two tiny jobs
  // (dir0 | dirPE, rgb) 36 workgroups each instead of 26-28 and the launch waited for dir0 | feature; 2 is worth -1.8 % of the
  // training step (tools/ab_train_step.py dw_unit_bias -1 2: 10.66 -> 10.46 ms; 0 / 1 / 3 within noise of it, 8: -0.8 %).
  int64_t units[DW_SPLIT_MAX_JOBS], total_units = 0;
  for (int j = 0; j < nj; ++j) {
    units[j] = jobs[j].nf + jobs[j].kf + bias;
    total_units += units[j];
  }
  // One workgroup per CU and launch (256), shares by largest remainder so that they sum to exactly 256: every
  // workgroup starts at once and, with the cost model above, ends at about the same time -- one prologue and one atomic
  // flush per CU instead of 6-16.  (tools/sweep_dw.py: 1.54 ms against 1.70 for the 192-sample pass, 0.52 against 0.66
  // for the 64-sample pass; with the old byte-only cost model 256 workgroups took 3.1 ms because the small jobs'
  // workgroups ran twice as long as the others.)
  int nw = 0;
  double frac[DW_SPLIT_MAX_JOBS];
  for (int j = 0; j < DW_SPLIT_MAX_JOBS; ++j) splits[j] = 0;
  for (int j = 0; j < nj; ++j) {
    const double share = (double)units[j] * target_wgs / (double)total_units;
    int64_t sp = (int64_t)share;
    frac[j] = share - (double)sp;
    if (sp < 1) { sp = 1; frac[j] = 0.0; }
    if (sp > max_splits) { sp = max_splits; frac[j] = 0.0; }
    splits[j] = (int)sp;
    nw += (int)sp;
  }
  while (nw < target_wgs) {                                     // hand out the remainder, largest fraction first
    int best = -1;
    for (int j = 0; j < nj; ++j)
      if (splits[j] < max_splits && (best < 0 || frac[j] > frac[best])) best = j;
    if (best < 0 || frac[best] <= 0.0) break;
    splits[best] += 1; frac[best] = 0.0; nw += 1;
  }
  while (nw > target_wgs) {                                     // (minimum-of-one bumps) take back from the largest
    int big = 0;
    for (int j = 1; j < nj; ++j) if (splits[j] > splits[big]) big = j;
    if (splits[big] <= 1) break;
    splits[big] -= 1; nw -= 1;
  }
  return nw;
}

}  // namespace nerf
