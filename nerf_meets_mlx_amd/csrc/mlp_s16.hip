// Split-bf16 training kernels of the fused 8 x 256 NeRF MLP for gfx950 (a11 and its adjoint at the reference's float32
// tolerance, on the bf16 matrix pipe): training forward with activation stores, dZ chain, dW / db.
//
// The reference computes NeRF.forward and its gradients in float32 (models/NeRF.py:201-243 under nn.value_and_grad,
// entrypoints/__test_nerf.py:240-293).  The fp32 MFMA (v_mfma_f32_32x32x2_f32, mlp32.hip) runs at 1/16 of the 16-bit rate.
// Here every float32 GEMM operand is carried as two bf16 numbers
//     x = hi + lo,   hi = bf16(x),  lo = bf16(x - hi)            (x - hi is exact in float32; 16 significand bits, float32's
// exponent range: gradients span far more than fp16's 30 binades, so the scaled-fp16 pairs of mlp22.hip do not apply here)
// and a product is evaluated as
//     a b  ~=  a_hi b_hi + a_hi b_lo + a_lo b_hi                 (the dropped a_lo b_lo is 2^-18 relative)
// = three v_mfma_f32_32x32x16_bf16 into ONE fp32 accumulator.  Everything else is the scheme of mlp.hip's training kernels
// (transposed layers, accumulator tile = next layer's B operand, weights streamed through the shared LDS ring by LDS-DMA,
// fragment-block stores, ReLU sign-bit words, split-K dW over fragment blocks with the sample axis as the MFMA K axis) with
// every stream doubled: (hi, lo) weight fragment pairs, hi and lo fragment blocks in the stores.
//
// The device code of the forward and the chain is mlp_s16_view.h, shared with mlp_s16f.hip, which instantiates the FOLDED form of the
// same kernels ("train_fold": mlp_s16.h); this unit holds the unfolded instantiations, the unfolded pack, the weight-gradient kernel
// and the host entry points of both forms.
//
// Forward / chain: one wave = 32 samples, ONE wave per SIMD (4 waves per workgroup): input and output layer, hi and lo, are
// 256 activation registers.  dW: 16 waves per workgroup as in mlp.hip, LDS stages of 16 samples (half a tile) so that four
// stages of hi + lo operands fit the CU's 160 KiB.
#include "mlp_s16_view.h"
#include "mlp_pack.h"

namespace nerf {
namespace s16 {

// ------------------------------------------------------------------------------------------
// packing: fp32 master parameters -> (hi, lo) bf16 fragment pairs in the 32x32x16 stream orders of mlp_index.h (mlp_pack.h)
// ------------------------------------------------------------------------------------------
// the transposed pair stream ends 1104 pairs in (4 of them zero padding), not at the bf16 stream's 1120
struct ViewPairPack : ViewPack { static constexpr int B_PADDED = s16::B_PADDED / 2; };
static_assert(ViewPairPack::B_PADDED >= L::B_TOTAL, "the padded stream holds every transposed fragment");

// ------------------------------------------------------------------------------------------
// dW: split-K GEMMs  dW[n][k] = sum_m dZ[n][m] H[k][m]  over hi / lo fragment blocks, samples = MFMA K
// ------------------------------------------------------------------------------------------
// LDS stage = 16 samples (half a sample tile, one MFMA k-step) of every operand fragment of the job, as "pair blocks" of
// 1 KiB: 16 sample rows x [even fragment 32 B | odd fragment 32 B] -- the two 16-feature fragments of one 32-wide operand
// tile side by side, so that a ds_read_b64_tr_b16 (4 sample rows x 2 fragments x 32 B per 32 lanes) covers 256 contiguous
// bytes: every bank once, no padding.  One LDS-DMA fills one pair block; the per-lane SOURCE address does the shuffle
// (lane i: row i >> 2, fragment (i >> 1) & 1, 16-byte half i & 1).  Blocks of a stage: dZ hi [n_tiles] | dZ lo [n_tiles] |
// H hi [k_tiles] | H lo [k_tiles]  <= 32 KiB.
#ifndef NERF_DWX
#define NERF_DWX 0            // timing-only builds (bit mask): 1 no DMAs, 2 no transposed reads, 4 no stage barrier, 8 no bias sums, 16 no MFMAs
#endif
#if NERF_DWX & 4
#define DW_BARRIER() do {} while (0)
#else
#define DW_BARRIER() __builtin_amdgcn_s_barrier()
#endif
constexpr int DW_WAVES = 16, DW_NPW = 2;                          // 2 x 2 output tiles per wave; 2 DMAs per wave per stage

__device__ __forceinline__ bf16x8 tr_pair(const char* blk, int hq, int fsel, int i16) {
  // A/B operand of v_mfma_f32_32x32x16_bf16 with K = samples 8 hq + (0..7) of the stage and row/col = feature (natural
  // order).  Lane i16 = 4 q + p of a 16-lane group addresses sample row q (and q + 4), feature piece p of fragment fsel.
  const int q = i16 >> 2, p = i16 & 3;
  const char* base = blk + 64 * (8 * hq + q) + 32 * fsel + 16 * (p & 1) + 8 * (p >> 1);
#if NERF_DWX & 2
  bf16x8 r; asm volatile("" : "=v"(r) : "v"(base)); return r;
#endif
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(base));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(base + 256));
  union { struct { s16x4 a, b; } s; bf16x8 v; } cvt;
  cvt.s.a = lo; cvt.s.b = hi;
  return cvt.v;
}

// ------------------------------------------------------------------------------------------
// the general dW kernel: 16 waves (4 x 4 waves of 2 x 2 output tiles), any job shape
// ------------------------------------------------------------------------------------------
// Since round 5 the 256 x 256 jobs run on mlp_dww.hip's one-wave-per-SIMD kernel; this one takes the narrow jobs (input layers,
// heads, the 2 x 64 model) and, with nerf_set_option("dw22_variant", 0), every job.
//  * Ring: a stage takes npairs KiB, the ring all 160 KiB of the CU: 5 stages for a 256 x 256 job, up to 8 for the narrow ones ("dw_ring_cap"; 6 / 8 / 16 measure the same in the training step).
//    ONE barrier per sample tile (two stages): the pair is waited for, the barrier frees the slots of the pair before it, every
//    stage whose slot is free is issued (two in steady state; ns - 2 stages stay in flight while a pair is processed), then both
//    half tiles are processed back to back -- the fixed cost of a stage boundary (barrier skew, the refill DMAs' blocked issue,
//    the LDS latency in front of the first MFMA) is paid once per 24 MFMAs of a wave instead of once per 12 (round 4's form: one
//    barrier per stage, 3.72-3.78 ms for the 786 k-sample launch; this form 3.35-3.45).  No padding DMAs: a wave waits with
//    vmcnt(its own DMAs per stage x the stages issued behind the pair).
//  * Jobs with k_tiles <= 2 number their waves column-major: the active waves then sit on four SIMDs instead of one.
//  * Every kernel argument the loop needs is copied into SGPRs in front of it: a scalar load inside the loop shares lgkmcnt with
//    the transposed reads and returns out of order, which makes hipcc wait with lgkmcnt(0) in front of every MFMA group (4.07 ms).
//  * Bias row sums (v_dot2c against (1, 1)) are spread over the waves of a row: (tile i, hi | lo part) c goes to wave column
//    c % (active columns), combined through the LDS once at the end in a fixed order.  The branches around them are kept branches
//    (empty asm): if-converted, every wave ran all sixteen v_dot2c and selected (+7 %).
// What bounds it (tools/probe_dw22_chain.py on the NERF_DWX timing-only builds, 786 k samples, all jobs): MFMAs alone 1.87 ms
// (the 256 x 256 workgroups at 0.78 us per stage, clock-limited), + barrier 0.06, + bias sums 0.3, + transposed reads 0.27 = 2.5 ms
// without a single DMA; the load skeleton alone 2.6-2.8 ms (6.3-6.7 TB/s); together 3.35-3.45: a wave of 128 registers cannot
// hold a second operand set, so reads and MFMAs of a stage are serial per wave and the four waves of a SIMD, in step behind the
// barrier, overlap them only by drifting apart.  An 8-wave form with two operand sets (round 5, removed) measured 3.54-3.72:
// two waves per SIMD in step leave the matrix pipe idle while both run their DMA / address / read instructions.  The 4-wave form
// (mlp_dww.hip) is what hides them.
constexpr int DW_LDS_BYTES = 160 * 1024;                  // the ring holds min(DW_LDS_BYTES / stage bytes, DwArgs.ring_cap) stages

// Jobs whose whole output is at most four tiles (the 2 x 64 model's layers, the view model's dir0 | dirPE and rgb jobs): with the
// 4 x 4 wave grid of 2 x 2 tiles ONE wave (or two) of sixteen has work, and the workgroup's rate is that wave's serial chain
// barrier -> reads -> wait -> MFMAs (measured: the 2 x 64 model's dW at 2.2 TB/s).  Here every wave is a pipeline of its own:
// wave w takes the stages w, w + 16, ... of the workgroup's sample range, moves them through its own 10 KiB of the LDS with its own
// DMAs and its own vmcnt wait -- no barrier in the loop, sixteen stages in flight per CU -- and accumulates its own copy of the
// NT x KT tiles; the sixteen copies are added through the LDS in a fixed binary tree at the end (bit-reproducible).
constexpr int DWP_WAVE_BYTES = 10 * 1024;
template <int NT, int KT, bool SPLIT>
__device__ __forceinline__ void dw_private(const DwArgs& a, const DwJob& jb, int tile_lo, int tile_hi, char* smem, int wv, int lane) {
  constexpr int NP = 2 * (NT + KT);                        // pair blocks per stage: dZ hi [NT] | dZ lo [NT] | H hi [KT] | H lo [KT]
  static_assert(NP * 1024 <= DWP_WAVE_BYTES && NT * KT <= 4, "wave-private dW: one stage per wave, at most four tiles");
  f32x16 acc[NT][KT];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int k = 0; k < KT; ++k)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][k][e] = 0.0f;
  float bsum[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) bsum[i] = 0.0f;
  const int g16 = lane >> 4, i16 = lane & 15, hq = g16 >> 1, fsel = g16 & 1;
  char* mine = smem + wv * DWP_WAVE_BYTES;
  const unsigned lds_mine = __builtin_amdgcn_readfirstlane(lds_addr_of(mine));
  const int src_row = lane >> 2, src_sel = (lane >> 1) & 1, src_half = lane & 1;
  const char* dzb = reinterpret_cast<const char*>(a.dz);
  const char* acb = reinterpret_cast<const char*>(a.acts);
  long long zstride_b = a.zstride * 16, astride_b = a.astride * 16;
  int z_lo = a.z_lo, a_lo = a.a_lo, dz_slot = jb.dz_slot, act_slot = jb.act_slot, nf = jb.nf, kf = jb.kf;
  asm volatile("" : "+s"(zstride_b), "+s"(astride_b), "+s"(z_lo), "+s"(a_lo), "+s"(dz_slot), "+s"(act_slot), "+s"(nf), "+s"(kf));
  // stages: SPLIT half tiles (two per sample tile: 16 samples of hi + lo blocks), bf16 whole sample tiles (samples 0-15 | 16-31 in
  // the blocks the lo parts occupy in the split form)
  const int ht_hi = SPLIT ? 2 * tile_hi : tile_hi;
  for (int ht = (SPLIT ? 2 * tile_lo : tile_lo) + wv; ht < ht_hi; ht += DW_WAVES) {
    // this wave's transposed reads of its previous stage are complete (every one feeds an MFMA above; the wait makes it explicit)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#if !(NERF_DWX & 1)
    const int64_t tile = SPLIT ? ht >> 1 : ht;
    const unsigned row_off0 = (unsigned)(32 * ((SPLIT ? 16 * (ht & 1) : 0) + src_row) + 16 * src_half);
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const bool is_z = i < 2 * NT;
      const int j = is_z ? i : i - 2 * NT, nt_ = is_z ? NT : KT;
      const int lo_part = j >= nt_ ? 1 : 0, t = lo_part ? j - nt_ : j;
      const int nfr = is_z ? nf : kf;
      int fr = 2 * t + src_sel; if (fr >= nfr) fr = nfr - 1;          // odd counts: rows past n_valid, never read back
      const int slot = (is_z ? dz_slot + (SPLIT ? lo_part * z_lo : 0) : act_slot + (SPLIT ? lo_part * a_lo : 0)) + fr;
      const unsigned row_off = row_off0 + (SPLIT ? 0 : 512 * lo_part);
      dma_frag_nt((is_z ? dzb + tile * zstride_b : acb + tile * astride_b) + (int64_t)slot * 1024 + row_off, lds_mine + i * 1024);
    }
#endif
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    bf16x8 bh[KT], bl[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) {
      bh[k] = tr_pair(mine + (2 * NT + k) * 1024, hq, fsel, i16);
      bl[k] = tr_pair(mine + (2 * NT + KT + k) * 1024, hq, fsel, i16);
    }
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const bf16x8 ah = tr_pair(mine + i * 1024, hq, fsel, i16);
      const bf16x8 al = tr_pair(mine + (NT + i) * 1024, hq, fsel, i16);
#if !(NERF_DWX & 8)
      const bf16x2 ones = {(__bf16)1.0f, (__bf16)1.0f};
#pragma unroll
      for (int j = 0; j < 8; j += 2) {
        const bf16x2 ph = {ah[j], ah[j + 1]}, pl = {al[j], al[j + 1]};
        bsum[i] = __builtin_amdgcn_fdot2_f32_bf16(pl, ones, bsum[i], false);
        bsum[i] = __builtin_amdgcn_fdot2_f32_bf16(ph, ones, bsum[i], false);
      }
#endif
#if NERF_DWX & 16
      asm volatile("" :: "v"(ah), "v"(al), "v"(bh[0]), "v"(bl[0]));
#else
#pragma unroll
      for (int k = 0; k < KT; ++k) {
        if (SPLIT) {
          acc[i][k] = mfma32(al, bh[k], acc[i][k]);
          acc[i][k] = mfma32(ah, bl[k], acc[i][k]);
          acc[i][k] = mfma32(ah, bh[k], acc[i][k]);
        } else {
          acc[i][k] = mfma32(ah, bh[k], acc[i][k]);
          acc[i][k] = mfma32(al, bl[k], acc[i][k]);
        }
      }
#endif
    }
  }
  // sixteen copies -> one, through the LDS: waves [h, 2h) hand theirs to waves [0, h), h = 8, 4, 2, 1 (fixed order)
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  float* xl = reinterpret_cast<float*>(smem);              // [giver][tile | bias row][register][lane]: 4 KiB per tile, 256 B per bias row
  constexpr int GIVER_FLOATS = (NT * KT * 16 + NT) * 64;
#pragma unroll 1
  for (int h = DW_WAVES / 2; h >= 1; h >>= 1) {
    __builtin_amdgcn_s_barrier();                          // the loop's reads (first round) / the previous round's reads are done
    if (wv >= h && wv < 2 * h) {
      float* dst = xl + (size_t)(wv - h) * GIVER_FLOATS + lane;
#pragma unroll
      for (int i = 0; i < NT; ++i) {
#pragma unroll
        for (int k = 0; k < KT; ++k)
#pragma unroll
          for (int e = 0; e < 16; ++e) dst[((i * KT + k) * 16 + e) * 64] = acc[i][k][e];
        dst[(NT * KT * 16 + i) * 64] = bsum[i];
      }
    }
    __builtin_amdgcn_s_barrier();
    if (wv < h) {
      const float* src = xl + (size_t)wv * GIVER_FLOATS + lane;
#pragma unroll
      for (int i = 0; i < NT; ++i) {
#pragma unroll
        for (int k = 0; k < KT; ++k)
#pragma unroll
          for (int e = 0; e < 16; ++e) acc[i][k][e] += src[((i * KT + k) * 16 + e) * 64];
        bsum[i] += src[(NT * KT * 16 + i) * 64];
      }
    }
  }
  if (wv != 0) return;
  const int rr = lane & 31, hh = lane >> 5;
  float* slot = a.partial + (size_t)blockIdx.x * DW_SLOT_FLOATS;
#pragma unroll
  for (int i = 0; i < NT; ++i) {
#pragma unroll
    for (int k = 0; k < KT; ++k) {
      float* tile = slot + (8 * i + k) * 1024;
#pragma unroll
      for (int e = 0; e < 16; ++e) tile[((e & 3) + 8 * (e >> 2) + 4 * hh) * 32 + rr] = acc[i][k][e];
    }
    if (jb.b_off >= 0) {
      const float tot = bsum[i] + __shfl_xor(bsum[i], 32, 64);      // the two sample halves of the k-step
      if (hh == 0) slot[64 * 1024 + 32 * i + rr] = tot;
    }
  }
}

template <bool SPLIT>
__global__ void __launch_bounds__(64 * DW_WAVES) s16_dw_kernel(DwArgs a) {
  char* smem = ring_smem;
  int bj = blockIdx.x, job_id = 0;
  while (bj >= a.splits[job_id]) { bj -= a.splits[job_id]; ++job_id; }
  const DwJob jb = a.jobs[job_id];
  const int tile_lo = (int)((int64_t)a.ntiles * bj / a.splits[job_id]);
  const int tile_hi = (int)((int64_t)a.ntiles * (bj + 1) / a.splits[job_id]);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n_tiles = (jb.nf + 1) >> 1, k_tiles = (jb.kf + 1) >> 1;
  const bool col_major = k_tiles <= 2;                    // see s16_dw_kernel
  const int wr = col_major ? (wv & 3) : (wv >> 2), wc = col_major ? (wv >> 2) : (wv & 3);
  const int npairs = 2 * (n_tiles + k_tiles);             // real pair blocks per stage (4 .. 32)
  if (a.private_max_tiles >= n_tiles * k_tiles && npairs * 1024 <= DWP_WAVE_BYTES) {       // tiny jobs: sixteen independent wave pipelines
    switch (8 * n_tiles + k_tiles) {
      case 8 * 1 + 1: dw_private<1, 1, SPLIT>(a, jb, tile_lo, tile_hi, smem, wv, lane); return;
      case 8 * 1 + 2: dw_private<1, 2, SPLIT>(a, jb, tile_lo, tile_hi, smem, wv, lane); return;
      case 8 * 1 + 3: dw_private<1, 3, SPLIT>(a, jb, tile_lo, tile_hi, smem, wv, lane); return;
      case 8 * 1 + 4: dw_private<1, 4, SPLIT>(a, jb, tile_lo, tile_hi, smem, wv, lane); return;
      case 8 * 2 + 1: dw_private<2, 1, SPLIT>(a, jb, tile_lo, tile_hi, smem, wv, lane); return;
      case 8 * 2 + 2: dw_private<2, 2, SPLIT>(a, jb, tile_lo, tile_hi, smem, wv, lane); return;
      case 8 * 3 + 1: dw_private<3, 1, SPLIT>(a, jb, tile_lo, tile_hi, smem, wv, lane); return;
      case 8 * 4 + 1: dw_private<4, 1, SPLIT>(a, jb, tile_lo, tile_hi, smem, wv, lane); return;
      default: break;
    }
  }
  const bool active = (wr * DW_NPW < n_tiles) && (wc * 2 < k_tiles);
  const int kc = (k_tiles + 1) >> 1;                      // active wave columns (1, 2 or 4)
  int stride = npairs * 1024, ns = DW_LDS_BYTES / stride;
  if (ns > a.ring_cap) ns = a.ring_cap;
  const int cnt_w = (wv < npairs ? 1 : 0) + (wv + DW_WAVES < npairs ? 1 : 0);   // this wave's DMAs per stage
  f32x16 acc[DW_NPW][2];
#pragma unroll
  for (int i = 0; i < DW_NPW; ++i)
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][k][e] = 0.0f;
  float bsum[2 * DW_NPW];                                 // [2 i + part]: part 0 = hi block, 1 = lo block of dZ tile i
  bool own[2 * DW_NPW];                                   // wave-uniform
#pragma unroll
  for (int c = 0; c < 2 * DW_NPW; ++c) { bsum[c] = 0.0f; own[c] = (c % kc) == wc && !(NERF_DWX & 8); }
  const int g16 = lane >> 4, i16 = lane & 15, hq = g16 >> 1, fsel = g16 & 1;
  const unsigned lds0 = __builtin_amdgcn_readfirstlane(lds_addr_of(smem));
  const int src_row = lane >> 2, src_sel = (lane >> 1) & 1, src_half = lane & 1;
  const char* dzb = reinterpret_cast<const char*>(a.dz);
  const char* acb = reinterpret_cast<const char*>(a.acts);
  long long zstride_b = a.zstride * 16, astride_b = a.astride * 16;
  int z_lo = a.z_lo, a_lo = a.a_lo, dz_slot = jb.dz_slot, act_slot = jb.act_slot, nf = jb.nf, kf = jb.kf;
  asm volatile("" : "+s"(zstride_b), "+s"(astride_b), "+s"(z_lo), "+s"(a_lo), "+s"(dz_slot), "+s"(act_slot), "+s"(nf), "+s"(kf),
               "+s"(stride), "+s"(ns));

  auto issue = [&](int ht, int slot) {
#if NERF_DWX & 1
    return;
#endif
    const unsigned st = lds0 + __builtin_amdgcn_readfirstlane(slot) * stride;
    const int64_t tile = SPLIT ? ht >> 1 : ht;
    const unsigned row_off0 = (unsigned)(32 * ((SPLIT ? 16 * (ht & 1) : 0) + src_row) + 16 * src_half);
#pragma unroll
    for (int k = 0; k < DW_NPW; ++k) {
      const int i = wv + DW_WAVES * k;                     // wave-uniform
      if (i < npairs) {
        const bool is_z = i < 2 * n_tiles;
        const int j = is_z ? i : i - 2 * n_tiles;
        const int nt_ = is_z ? n_tiles : k_tiles;
        const int lo_part = j >= nt_ ? 1 : 0;
        const int t = lo_part ? j - nt_ : j;
        const int nfr = is_z ? nf : kf;
        int fr = 2 * t + src_sel; if (fr >= nfr) fr = nfr - 1;
        // part 1 of an operand: SPLIT the lo blocks (z_lo / a_lo slots further), bf16 samples 16..31 of the same fragments
        const int slot_ = (is_z ? dz_slot + (SPLIT ? lo_part * z_lo : 0) : act_slot + (SPLIT ? lo_part * a_lo : 0)) + fr;
        const unsigned row_off = row_off0 + (SPLIT ? 0 : 512 * lo_part);
        const char* src = (is_z ? dzb + tile * zstride_b : acb + tile * astride_b) + (int64_t)slot_ * 1024 + row_off;
        dma_frag_nt(src, st + i * 1024);
      }
    }
  };
  auto process = [&](const char* st) {
    if (active) {
      bf16x8 bh[2], bl[2];
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int kt = wc * 2 + k;
        const int b = 2 * n_tiles + (kt < k_tiles ? kt : 0);
        bh[k] = tr_pair(st + b * 1024, hq, fsel, i16);
        bl[k] = tr_pair(st + (b + k_tiles) * 1024, hq, fsel, i16);
      }
#pragma unroll
      for (int i = 0; i < DW_NPW; ++i) {
        const int nt = wr * DW_NPW + i;
        const int b = nt < n_tiles ? nt : 0;
        const bf16x8 ah = tr_pair(st + b * 1024, hq, fsel, i16);
        const bf16x8 al = tr_pair(st + (b + n_tiles) * 1024, hq, fsel, i16);
        const bf16x2 ones = {(__bf16)1.0f, (__bf16)1.0f};
        // bias gradient = row sums of dZ: v_dot2c_f32_bf16 against (1, 1).  (The empty asm keeps the wave-uniform branch a branch:
        // hipcc otherwise runs all sixteen v_dot2c on every wave and selects with v_cndmask.)
        if (own[2 * i]) {
          asm volatile("" ::: "memory");
#pragma unroll
          for (int j = 0; j < 8; j += 2) { const bf16x2 q = {ah[j], ah[j + 1]}; bsum[2 * i] = __builtin_amdgcn_fdot2_f32_bf16(q, ones, bsum[2 * i], false); }
        }
        if (own[2 * i + 1]) {
          asm volatile("" ::: "memory");
#pragma unroll
          for (int j = 0; j < 8; j += 2) { const bf16x2 q = {al[j], al[j + 1]}; bsum[2 * i + 1] = __builtin_amdgcn_fdot2_f32_bf16(q, ones, bsum[2 * i + 1], false); }
        }
#if NERF_DWX & 16
        asm volatile("" :: "v"(ah), "v"(al), "v"(bh[0]), "v"(bl[0]), "v"(bh[1]), "v"(bl[1]));
#else
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          if (SPLIT) {                         // lo hi + hi lo + hi hi
            acc[i][k] = mfma32(al, bh[k], acc[i][k]);
            acc[i][k] = mfma32(ah, bl[k], acc[i][k]);
            acc[i][k] = mfma32(ah, bh[k], acc[i][k]);
          } else {                             // samples 0-15, then 16-31
            acc[i][k] = mfma32(ah, bh[k], acc[i][k]);
            acc[i][k] = mfma32(al, bl[k], acc[i][k]);
          }
        }
#endif
      }
    }
  };
  // wait until this wave's DMAs of everything but the `younger` most recently issued stages have landed (wave-uniform, <= 14 stages
  // x <= 2 DMAs), and until its own transposed reads of the previous pair are complete
  auto wait_landed = [&](int younger) {
    switch (younger * cnt_w) {
#define NERF_VM_CASE(N) case N: asm volatile("s_waitcnt vmcnt(" #N ") lgkmcnt(0)" ::: "memory"); break;
      NERF_VM_CASE(0) NERF_VM_CASE(1) NERF_VM_CASE(2) NERF_VM_CASE(3) NERF_VM_CASE(4) NERF_VM_CASE(5) NERF_VM_CASE(6) NERF_VM_CASE(7)
      NERF_VM_CASE(8) NERF_VM_CASE(9) NERF_VM_CASE(10) NERF_VM_CASE(11) NERF_VM_CASE(12) NERF_VM_CASE(13) NERF_VM_CASE(14)
      NERF_VM_CASE(16) NERF_VM_CASE(18) NERF_VM_CASE(20) NERF_VM_CASE(22) NERF_VM_CASE(24) NERF_VM_CASE(26) NERF_VM_CASE(28)
#undef NERF_VM_CASE
      default: asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); break;
    }
  };
  // stages of this workgroup: SPLIT half tiles (two per sample tile, n even), bf16 sample tiles (n may be odd: the last pair is single)
  const int ht_lo = SPLIT ? 2 * tile_lo : tile_lo, n = SPLIT ? 2 * (tile_hi - tile_lo) : tile_hi - tile_lo;
  int issued = 0, slot_i = 0, slot_p = 0;                  // stages issued so far; the slot the next issue / the next process uses
  for (; issued < ns && issued < n; ++issued) { issue(ht_lo + issued, slot_i); slot_i = slot_i + 1 == ns ? 0 : slot_i + 1; }
  for (int p = 0; p < n; p += 2) {
    wait_landed(issued - (p + 2 < n ? p + 2 : n));         // stages p, p + 1 landed (this wave's part)
    DW_BARRIER();                                          // ... for every wave; every wave is done with the stages before p
#pragma unroll
    for (int k = 0; k < 2; ++k)                            // the slots of stages < p are free: stage s may go once s - ns < p
      if (issued < n && issued - ns < p) { issue(ht_lo + issued, slot_i); slot_i = slot_i + 1 == ns ? 0 : slot_i + 1; ++issued; }
    process(smem + slot_p * stride); slot_p = slot_p + 1 == ns ? 0 : slot_p + 1;
    if (SPLIT || p + 1 < n) { process(smem + slot_p * stride); slot_p = slot_p + 1 == ns ? 0 : slot_p + 1; }
  }
  // bias partial sums of a wave row -> its wc == 0 wave, through the LDS (every wave takes part in the two barriers)
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  float* xb = reinterpret_cast<float*>(smem);              // [wr][c][lane]
#pragma unroll
  for (int c = 0; c < 2 * DW_NPW; ++c)
    if (own[c] && active) xb[(wr * 2 * DW_NPW + c) * 64 + lane] = bsum[c];
  __builtin_amdgcn_s_barrier();
  if (!active) return;
  const int rr = lane & 31, hh = lane >> 5;
  float* slot = a.partial + (size_t)blockIdx.x * DW_SLOT_FLOATS;
#pragma unroll
  for (int i = 0; i < DW_NPW; ++i) {
    const int nt = wr * DW_NPW + i;
    if (nt >= n_tiles) continue;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int kt = wc * 2 + k;
      if (kt >= k_tiles) continue;
      float* tile = slot + (8 * nt + kt) * 1024;
#pragma unroll
      for (int e = 0; e < 16; ++e) tile[((e & 3) + 8 * (e >> 2) + 4 * hh) * 32 + rr] = acc[i][k][e];      // 128 B per half wave
    }
    if (wc == 0 && jb.b_off >= 0) {
      const float lo = xb[(wr * 2 * DW_NPW + 2 * i + 1) * 64 + lane], hi = xb[(wr * 2 * DW_NPW + 2 * i) * 64 + lane];
      const float t = lo + hi;
      const float tot = t + __shfl_xor(t, 32, 64);         // the two sample halves of the k-step
      if (hh == 0) slot[64 * 1024 + 32 * nt + rr] = tot;
    }
  }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------

int pack(const float* params, void* packed_s16, bool fold, hipStream_t s) {
  bf16x8* wf = static_cast<bf16x8*>(packed_s16);
  if (fold) return pack_folded(params, packed_s16, s);       // mlp_s16f.hip
  return launch<pack_streams_kernel<ViewPairPack, SplitBf16, false>>("nerf_mlp_pack (split-bf16 image)", dim3(pack_blocks<ViewPairPack, false>()),
                                                                     dim3(256), 0, s, params, wf, wf + (size_t)F_FRAGS * 64, nullptr, 0);
}

int forward(const void* packed_s16, const float* bias_slots, const float* x, const float* rays, const float* z, int64_t M,
            int n, int freq_mode, float* out, void* acts, int64_t astride16, int persistent_wgs, bool fold, hipStream_t s) {
  if (fold)                                                  // the folded kernels are a unit of their own: mlp_s16f.hip
    return forward_folded(packed_s16, bias_slots, x, rays, z, M, n, freq_mode, out, acts, astride16, persistent_wgs, s);
  FwdArgs a;
  a.queue = passq_slot();
  a.wf = reinterpret_cast<const bf16x8*>(packed_s16);
  a.bias = bias_slots;
  a.x = x; a.rays = rays; a.z = z; a.M = M; a.n = n; a.out = out; a.acts = acts; a.astride = astride16;
  fill_freqs(a.fr.pos, a.fr.dir, freq_mode);
  const int64_t nsuper = ((M + 31) / 32 + NW - 1) / NW;
  return with_bool(x != nullptr, [&](auto rows) {          // MODE 0: embedded rows, 1: rays + depths
    return launch<s16_fwd_kernel<decltype(rows)::value ? 0 : 1, false>>("mlp training forward (split bf16)", dim3(persistent_grid(nsuper, persistent_wgs)),
                                                                         dim3(64 * NW), FwdRing::LDS_BYTES, s, a);
  });
}

int backward_chain(const void* packed_s16, const void* acts, const float* d_raw, int64_t M, void* dz, int64_t astride16,
                   int64_t zstride16, int persistent_wgs, bool fold, hipStream_t s) {
  if (fold) return backward_chain_folded(packed_s16, acts, d_raw, M, dz, astride16, zstride16, persistent_wgs, s);
  BwdArgs b;
  b.queue = passq_slot();
  b.wb = reinterpret_cast<const bf16x8*>(static_cast<const char*>(packed_s16) + (size_t)F_FRAGS * 1024);
  b.acts = acts; b.d_raw = d_raw; b.M = M; b.dz = dz; b.astride = astride16; b.zstride = zstride16;
  const int64_t nsuper = ((M + 31) / 32 + NW - 1) / NW;
  return launch<s16_bwd_kernel<false>>("mlp backward chain (split bf16)", dim3(persistent_grid(nsuper, persistent_wgs)), dim3(64 * NW),
                                       BwdRing::LDS_BYTES, s, b);
}

int g_dw_variant = 1;          // nerf_set_option("dw22_variant"): 1 (default) 256 x 256 jobs on mlp_dww.hip's kernel, the others here; 0 every job here

int launch_dw_kernel(const DwArgs& d, int workgroups, bool split_bf16, hipStream_t s) {
  return with_bool(split_bf16, [&](auto split) {
    return launch<s16_dw_kernel<decltype(split)::value>>(split_bf16 ? "mlp dW (split bf16)" : "mlp dW (bf16)", dim3(workgroups), dim3(64 * DW_WAVES),
                                                         DW_LDS_BYTES, s, d);
  });
}

}  // namespace s16
}  // namespace nerf
