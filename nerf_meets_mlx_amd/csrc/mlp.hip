// Fully-fused 8x256 NeRF MLP for gfx950 (a11, a12 / K3, K4, K5): positional encoding +
// 12 linear layers in ONE kernel, bf16 MFMA (v_mfma_f32_32x32x16_bf16) with fp32 accumulate.
//
// Orientation.  Every layer is computed TRANSPOSED:  H_out^T[n][m] = sum_k W[n][k] H_in^T[k][m]
// with A = W (rows n, nn.Linear's [out][in] layout gives 8 contiguous k per lane) and
// B = H_in^T (k on the lane half / element, sample m on lane&31).  The accumulator tile then
// has the SAMPLE on the lane and the output FEATURES in the 16 registers, which -- after
// bias + ReLU + cvt to bf16 -- is already the B operand of the next layer (the k order inside
// a 16-step is permuted: element j of lane half h is feature 16s + 8(j>>2) + 4h + (j&3); the
// weight fragments are packed in that order by nerf_mlp_pack).  So a wave keeps its 32 (or
// 64) samples in registers through all layers: no LDS round trip, no HBM traffic for
// activations in inference, and weights stream as fully coalesced 1 KiB fragments.
//
// Training stores the per-layer bf16 activations as 1 KiB "fragment blocks" (32 samples x
// 16 features, lane (r,h) at byte 32r+16h) which the backward chain kernel reloads as ReLU
// masks and the dW kernel consumes through LDS with ds_read_b64_tr_b16 (the sample axis
// becomes the MFMA K axis there).
//
// Map of the file: layouts + packing (namespace L) | weight sources (GlobalW: L1, RingW: LDS ring fed by LDS-DMA,
// LdsW: LDS-resident) | layer_fwd / fwd_tiles and the 32x32x16 forward kernels | the 16x16x32 render forward
// (mlp_fwd_ring16_kernel, the default for inference) | layer_bwd / bwd_tiles (dZ chain) | mlp_dw_kernel (dW / db) |
// second layout: image-fitting model (namespace LI) | third layout: 2 x 64 model of configs[4] (namespace LN) |
// C ABI entry points.
#include "common.h"
#include "mlp_ring.h"
#include "mlp_layout.h"
#include "mlp_frag.h"
#include "mlp_arch2.h"
#include "mlp_input2.h"
#include "mlp_pack.h"
#include "hash_common.h"
#include "mlp_params.h"
#include "mlp_model.h"
#include "dw_split.h"
#include <limits.h>
#include <string.h>


namespace nerf {

extern int g_hash_combine_max_res;        // encode.hip


// static layout (namespace L), kperm: mlp_layout.h

// ------------------------------------------------------------------------------------------
// weight packing: fp32 master parameters -> bf16 MFMA fragments (+ fp32 bias slots)
// ------------------------------------------------------------------------------------------
// the index maps: mlp_index.h (ViewPack); the routine: mlp_pack.h

// ------------------------------------------------------------------------------------------
// positional encoding straight into B-operand fragments
// ------------------------------------------------------------------------------------------


// channel order, evaluators, encoders, row readers, sample loader: mlp_input.h (here: SinRevFract; CvtBf16 in the 32x32x16 chains, PackBf16 in the 16x16x32 render kernel)

// weight sources (GlobalW: L1, RingW: LDS ring fed by LDS-DMA), FwdArgs, PeFreq: mlp_ring.h
// ------------------------------------------------------------------------------------------
// one linear layer on register-resident activations
// ------------------------------------------------------------------------------------------
// fragment blocks, packed-pair helpers, epilogue schedule, DwJob / DwArgs: mlp_frag.h

// out[t][2 nt + s] = act( W[nt-tile] . in[t] + bias );  fragments fbase + nt*KS + ks of the stream
template <int ST, int KS, int NT, bool RELU, bool MASKOUT, class WS, class SINK = NoSink>
__device__ __forceinline__ void layer_fwd(WS& ws, int fbase, int bias_slot, const bf16x8 (&in)[ST][KS],
                                          bf16x8 (&out)[ST][2 * NT], u32x4 (&mask)[ST], int lane,
                                          const SINK& sink = SINK()) {
  const int h = lane >> 5;
  f32x16 prev[ST];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    f32x16 acc[ST];
    acc_init_bias(acc[0], ws, bias_slot + 32 * nt, h);
#pragma unroll
    for (int t = 1; t < ST; ++t) acc[t] = acc[0];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const bf16x8 a = next_frag(ws, fbase + nt * KS + ks, lane);
#pragma unroll
      for (int t = 0; t < ST; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, in[t][ks], acc[t], 0, 0, 0);
      if (nt > 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (quarter_pos(KS, q) == ks) {
#pragma unroll
            for (int t = 0; t < ST; ++t) {
              finish_quarter<RELU, MASKOUT>(prev[t], q, nt - 1, out[t][2 * nt - 2], out[t][2 * nt - 1], mask[t]);
              if (q == 3) { sink.put(t, 2 * nt - 2, out[t][2 * nt - 2]); sink.put(t, 2 * nt - 1, out[t][2 * nt - 1]); }
            }
          }
      }
    }
#pragma unroll
    for (int t = 0; t < ST; ++t) prev[t] = acc[t];
  }
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int t = 0; t < ST; ++t)
      finish_quarter<RELU, MASKOUT>(prev[t], q, NT - 1, out[t][2 * NT - 2], out[t][2 * NT - 1], mask[t]);
#pragma unroll
  for (int t = 0; t < ST; ++t) { sink.put(t, 2 * NT - 2, out[t][2 * NT - 2]); sink.put(t, 2 * NT - 1, out[t][2 * NT - 1]); }
}


// All 12 layers for ST sample tiles of this wave (tile0 .. tile0+ST-1).  Tiles >= ntiles are computed on clamped
// inputs and never stored, so every wave runs the same instruction stream (the ring needs that).
// MODE 0: embedded rows;  MODE 1: rays + z with fused positional encodings
template <int ST, int MODE, bool STORE, class WS>
__device__ __forceinline__ void fwd_tiles(const FwdArgs& a, WS& ws, int64_t tile0, int64_t ntiles, int lane, PassQueue* pq = nullptr) {
  const int r = lane & 31, h = lane >> 5;
  bf16x8 pe[ST][4], dpe[ST][2];
  if (pq) pq->ask(ws_wave(ws), lane);          // dynamic pass queue (mlp_ring.h): before this pass's input loads
#pragma unroll
  for (int t = 0; t < ST; ++t) {
    int64_t tile = tile0 + t; if (tile >= ntiles) tile = ntiles - 1;
    const int64_t m = clamp_sample(tile * 32 + r, a.M);
    if (MODE == 0) {
      const float* row = a.x + m * 90;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) row_pairs<CvtBf16>(row, ks, h, 63, pe[t][ks]);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) row_pairs<CvtBf16>(row + 63, ks, h, 27, dpe[t][ks]);
    } else {
      const Sample sm = load_sample(a.rays, a.z, m, a.n);
#if NERF_ABLATE == 3          // timing-only build 3: no positional-encoding arithmetic
      for (int q = 0; q < 4; ++q) for (int j = 0; j < 8; ++j) pe[t][q][j] = (__bf16)sm.p[j % 3];
      for (int q = 0; q < 2; ++q) for (int j = 0; j < 8; ++j) dpe[t][q][j] = (__bf16)sm.d[j % 3];
      if (false)
#endif
      {
      encode_pairs<SinRevFract, CvtBf16, 0, 63, 10>(sm.p, a.fr.pos, h, pe[t][0]); encode_pairs<SinRevFract, CvtBf16, 1, 63, 10>(sm.p, a.fr.pos, h, pe[t][1]);
      encode_pairs<SinRevFract, CvtBf16, 2, 63, 10>(sm.p, a.fr.pos, h, pe[t][2]); encode_pairs<SinRevFract, CvtBf16, 3, 63, 10>(sm.p, a.fr.pos, h, pe[t][3]);
      encode_pairs<SinRevFract, CvtBf16, 0, 27, 4>(sm.d, a.fr.dir, h, dpe[t][0]); encode_pairs<SinRevFract, CvtBf16, 1, 27, 4>(sm.d, a.fr.dir, h, dpe[t][1]);
      }
    }
  }
  if (pq) pq->publish(ws_wave(ws));
  int bad[ST];                      // non-finite inputs of this lane's sample (mlp_frag.h: nonfinite_flags), used at the output store
#pragma unroll
  for (int t = 0; t < ST; ++t)
  {
    bad[t] = nonfinite_flags<32>(nonfinite_bits(pe[t][0]) | nonfinite_bits(pe[t][1]) | nonfinite_bits(pe[t][2]) | nonfinite_bits(pe[t][3]),
                                 nonfinite_bits(dpe[t][0]) | nonfinite_bits(dpe[t][1]));
    // computed HERE, at the head of the pass.  Left to the scheduler, this arithmetic was sunk into the layer epilogues of the 2 x 64
    // training forward, whose layer-0 ReLU sign words then lost bits (tests: test_weight_gradients_of_the_two_dw_launch_forms_agree
    // [*-small-16]; the ISA of the interleaved form showed nothing wrong, the pinned form is bit-identical to the build without flags)
    asm volatile("" : "+v"(bad[t]));
  }
#define store(slot0, t, frags, count) \
  do { if (STORE) { store_frags<count>(a.acts, tile0 + (t), a.astride, slot0, frags, r, h); ws.note_stores(count); } } while (0)
#pragma unroll
  for (int t = 0; t < ST; ++t) { store(L::A_PE, t, pe[t], 4); store(L::A_DPE, t, dpe[t], 2); }

  bf16x8 ha[ST][16], hb[ST][16];
  u32x4 mk[ST];
#define SINK(slot0) FragSink<STORE>{a.acts, tile0, a.astride, slot0, r, h}
#define MASK_BEGIN() do { _Pragma("unroll") for (int t = 0; t < ST; ++t) mk[t] = u32x4{0u, 0u, 0u, 0u}; } while (0)
#define MASK_STORE(layer) do { if (STORE) { _Pragma("unroll") for (int t = 0; t < ST; ++t) \
    *reinterpret_cast<u32x4*>(frag_ptr(a.acts, tile0 + t, a.astride, L::A_MASK + (layer), r, h)) = mk[t]; ws.note_stores(ST); } } while (0)
  MASK_BEGIN();
  layer_fwd<ST, 4, 8, true, STORE>(ws, L::F_L0, 0, pe, ha, mk, lane, SINK(L::A_H0));
  MASK_STORE(0);
  // pos1..pos4 (ping-pong)
  MASK_BEGIN();
  layer_fwd<ST, 16, 8, true, STORE>(ws, L::F_L1 + 0 * 128, 256, ha, hb, mk, lane, SINK(L::A_H0 + 16));
  MASK_STORE(1);
  MASK_BEGIN();
  layer_fwd<ST, 16, 8, true, STORE>(ws, L::F_L1 + 1 * 128, 512, hb, ha, mk, lane, SINK(L::A_H0 + 32));
  MASK_STORE(2);
  MASK_BEGIN();
  layer_fwd<ST, 16, 8, true, STORE>(ws, L::F_L1 + 2 * 128, 768, ha, hb, mk, lane, SINK(L::A_H0 + 48));
  MASK_STORE(3);
  MASK_BEGIN();
  layer_fwd<ST, 16, 8, true, STORE>(ws, L::F_L1 + 3 * 128, 1024, hb, ha, mk, lane, SINK(L::A_H0 + 64));
  MASK_STORE(4);
  // pos5 on concat[input_pos, h]  (models/NeRF.py:224-225)
  {
    bf16x8 cat[ST][20];
#pragma unroll
    for (int t = 0; t < ST; ++t) {
      if (STORE && is_ring<WS>::value) {   // register relief in the training ring kernel: the encoding was just stored
#pragma unroll
        for (int k = 0; k < 4; ++k) pe[t][k] = *frag_ptr(a.acts, tile0 + t, a.astride, L::A_PE + k, r, h);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) cat[t][k] = pe[t][k];
#pragma unroll
      for (int k = 0; k < 16; ++k) cat[t][4 + k] = ha[t][k];
    }
    MASK_BEGIN();
    layer_fwd<ST, 20, 8, true, STORE>(ws, L::F_L5, 1280, cat, hb, mk, lane, SINK(L::A_H0 + 80));
    MASK_STORE(5);
  }
  MASK_BEGIN();
  layer_fwd<ST, 16, 8, true, STORE>(ws, L::F_L6, 1536, hb, ha, mk, lane, SINK(L::A_H0 + 96));
  MASK_STORE(6);
  MASK_BEGIN();
  layer_fwd<ST, 16, 8, true, STORE>(ws, L::F_L7, 1792, ha, hb, mk, lane, SINK(L::A_H0 + 112));
  MASK_STORE(7);
  // feature (no activation) and alpha (row 0 of a ninth tile)   models/NeRF.py:229-231
  layer_fwd<ST, 16, 8, false, false>(ws, L::F_FA, L::BI_FEAT, hb, ha, mk, lane, SINK(L::A_FEAT));
  float alpha[ST];
  {
    f32x16 acc[ST];
    acc_init_bias(acc[0], ws, L::BI_ALPHA, h);
#pragma unroll
    for (int t = 1; t < ST; ++t) acc[t] = acc[0];
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
      const bf16x8 wa = next_frag(ws, L::F_FA + 128 + ks, lane);
#pragma unroll
      for (int t = 0; t < ST; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wa, hb[t][ks], acc[t], 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < ST; ++t) alpha[t] = acc[t][0];
  }
  // view branch: relu(Linear([feature, input_dir]))  then rgb   models/NeRF.py:232-238
  bf16x8 hd[ST][8];
  {
    bf16x8 cat[ST][18];
#pragma unroll
    for (int t = 0; t < ST; ++t) {
#pragma unroll
      for (int k = 0; k < 16; ++k) cat[t][k] = ha[t][k];
      if (STORE && is_ring<WS>::value) {
        dpe[t][0] = *frag_ptr(a.acts, tile0 + t, a.astride, L::A_DPE, r, h);
        dpe[t][1] = *frag_ptr(a.acts, tile0 + t, a.astride, L::A_DPE + 1, r, h);
      }
      cat[t][16] = dpe[t][0]; cat[t][17] = dpe[t][1];
    }
    MASK_BEGIN();
    layer_fwd<ST, 18, 4, true, STORE>(ws, L::F_DIR, L::BI_DIR, cat, hd, mk, lane, SINK(L::A_HD));
    MASK_STORE(8);
  }
  {
    f32x16 acc[ST];
    acc_init_bias(acc[0], ws, L::BI_RGB, h);
#pragma unroll
    for (int t = 1; t < ST; ++t) acc[t] = acc[0];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const bf16x8 wr = next_frag(ws, L::F_RGB + ks, lane);
#pragma unroll
      for (int t = 0; t < ST; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wr, hd[t][ks], acc[t], 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < ST; ++t) {
      const int64_t m = (tile0 + t) * 32 + r;
      if (h == 0 && tile0 + t < ntiles && m < a.M) {
        float4 o; o.x = acc[t][0]; o.y = acc[t][1]; o.z = acc[t][2]; o.w = alpha[t];     // [rgb, alpha] raw
        *reinterpret_cast<float4*>(a.out + m * 4) = poison_raw(o, bad[t]);
      }
    }
  }
#undef store
#undef SINK
#undef MASK_BEGIN
#undef MASK_STORE
}

// variants 1 / 2: 4 independent waves per workgroup, weights through L1
template <int ST, int MODE, bool STORE>
__global__ void __launch_bounds__(256, (ST == 1 ? 2 : 1)) mlp_fwd_kernel(FwdArgs a) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t tile0 = ((int64_t)blockIdx.x * 4 + wv) * ST;
  const int64_t ntiles = (a.M + 31) >> 5;
  if (tile0 >= ntiles) return;
  GlobalW ws{a.wf + lane, a.bias};
  fwd_tiles<ST, MODE, STORE>(a, ws, tile0, ntiles, lane);
}


// variant 3: persistent workgroups of 8 waves x 32 samples, weights through the shared LDS ring
constexpr int F_CHUNKS = L::F_TOTAL / RING_CHUNK;     // 37
static_assert(F_CHUNKS * RING_CHUNK == L::F_TOTAL, "forward stream must be whole chunks");
constexpr int SPLIT_NW = 4, SPLIT_CHUNK = 16;         // the two-workgroups-per-CU form of the training kernels
constexpr int SPLIT_LDS_BYTES = RING_STAGES * SPLIT_CHUNK * 1024 + 2560 * 4;      // 75 776 B: two fit the 160 KiB of a CU

#ifdef NERF_CLOCK_STAMP
// Diagnostic build only (tools/probe_clock.py): in-kernel clock = d(s_memtime) / d(s_memrealtime) x 100 MHz
// (MI355X_MICROARCH "DVFS" item 6).  Stamps go to a buffer of their own; no output depends on them.
__device__ unsigned long long g_stamps[4096][4];
#define NERF_STAMP_BEGIN() const unsigned long long st_t0 = __builtin_amdgcn_s_memtime(), st_r0 = __builtin_amdgcn_s_memrealtime(); unsigned long long st_passes = 0
#define NERF_STAMP_PASS() ++st_passes
#define NERF_STAMP_END() do { if (threadIdx.x == 0 && blockIdx.x < 4096) { g_stamps[blockIdx.x][0] = __builtin_amdgcn_s_memtime() - st_t0; \
  g_stamps[blockIdx.x][1] = __builtin_amdgcn_s_memrealtime() - st_r0; g_stamps[blockIdx.x][2] = st_passes; g_stamps[blockIdx.x][3] = 1; } } while (0)
#else
#define NERF_STAMP_BEGIN()
#define NERF_STAMP_PASS()
#define NERF_STAMP_END()
#endif
// NW = 8, CHUNK = 32: ONE persistent workgroup of 8 waves per CU behind one 128 KiB ring (all 8 waves in lockstep).
// NW = 4, CHUNK = 16: TWO independent workgroups of 4 waves per CU, each behind its own 64 KiB ring: the two waves of a
// SIMD then belong to different workgroups and are not tied to one ring barrier, so the fragment stores of one group
// (the CU's store path takes ~29 cycles per KiB, and a wave blocked on a store issues no MFMA) can run under the MFMAs
// of the other; the price is each group streaming the whole weight image for 128 instead of 256 samples.
template <int MODE, bool STORE, int NW = 8, int CHUNK = RING_CHUNK>
__global__ void __launch_bounds__(64 * NW, 2) mlp_fwd_ring_kernel(FwdArgs a) {
  static_assert(L::F_TOTAL % CHUNK == 0, "forward stream must be whole chunks");
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t ntiles = (a.M + 31) >> 5;
  const int64_t nsuper = (ntiles + NW - 1) / NW;
  typedef RingW<L::F_TOTAL / CHUNK, L::F_TOTAL, (STORE ? 2 : 4), NW, CHUNK> Ring;
  Ring ws;
  ws.wsrc = reinterpret_cast<const char*>(a.wf);
  ws.lane16 = 16 * lane;
  ws.lds0 = __builtin_amdgcn_readfirstlane(lds_addr_of(ring_smem));
  ws.wv = wv;
  ws.start(lane);
  ring_load_bias(a.bias, L::BI_TOTAL, Ring::BIAS_OFF);
  __syncthreads();
  NERF_STAMP_BEGIN();
  PassQueue pq;                                         // dynamic pass queue (mlp_ring.h); a.queue == nullptr: static split
  pq.init(a.queue, ws.lds0 + Ring::BIAS_OFF);
  for (int64_t sp = blockIdx.x; sp < nsuper;) {
    int ln = lane;
    asm volatile("" : "+v"(ln));          // lane-derived values are recomputed per pass, not hoisted and spilled
    ws.new_pass();
    fwd_tiles<1, MODE, STORE>(a, ws, sp * NW + wv, ntiles, ln, &pq);
    NERF_STAMP_PASS();
    sp = pq.next(sp);
  }
  NERF_STAMP_END();
  ws.drain();                                           // the ring always runs 3 chunks ahead
  pq.leave();
}


// ==========================================================================================
// Variant 4 (inference only): the same register-resident chain on v_mfma_f32_16x16x32_bf16.
// The guide measures a higher held clock for this shape (MI355X_MICROARCH "DVFS give-back" item 7).  A wave still
// carries 32 samples, as two 16-sample column tiles that share every A fragment (16 output features x 32 k).
// Accumulator: col = lane&15 (sample), row = 4 (lane>>4) + reg; two stacked 16-feature tiles give the next layer's
// B fragment, element j of lane group g = feature 16 (j>>2) + 4 g + (j&3) of the 32-feature k-step.
// ==========================================================================================
// L16 stream offsets, kperm16, pos_chan16 / dir_chan16, fwd_src16: mlp_layout.h
// the whole bf16 image in ONE launch (was two: at N_rand = 1024 the ~30 five-microsecond launches of an iteration are a tenth
// of it): blocks [0, PACK_BLOCKS) build the 32x32x16 forward / backward streams and the bias slots, the rest the 16x16x32
// forward stream of the render kernels
constexpr int PACK_BLOCKS = pack_blocks<ViewPack, true>(), PACK16_BLOCKS = L::F16_PADDED * 64 / 256;
__global__ void __launch_bounds__(256) pack_kernel(const float* __restrict__ p, bf16x8* __restrict__ wf,
                                                   bf16x8* __restrict__ wb, float* __restrict__ bias,
                                                   bf16x8* __restrict__ w16) {
  if (blockIdx.x < PACK_BLOCKS) {
    pack_streams<ViewPack, CvtBf16, true>(blockIdx.x * 256 + threadIdx.x, p, wf, wb, bias, 0);
    return;
  }
  const int t = (blockIdx.x - PACK_BLOCKS) * 256 + threadIdx.x;
  if (t >= L::F16_PADDED * 64) return;
  const int f = t >> 6, lane = t & 63;
  bf16x8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = (__bf16)fwd_src16(p, f, lane & 15, lane >> 4, j);
  w16[t] = v;
}

constexpr int RING16_LDS_BYTES = RING_LDS_BYTES;
#ifndef NERF_BF16_IGLP
#define NERF_BF16_IGLP 0      // __builtin_amdgcn_iglp_opt strategy of the bf16 render layers (as in mlp22.hip: 4.79 -> 4.71 ms per fine pass); -1: none
#endif
// out[s][nt>>1] (elements 4 (nt&1) + i) = act( W[16-row tile nt] . in[s] + bias ), s = 0..NS-1 sample tiles of 16.
template <int NS, int KS, int NT, bool RELU, class WS>
__device__ __forceinline__ void layer_fwd16(WS& ws, int fbase, int bias_slot, const bf16x8 (&in)[NS][KS],
                                            bf16x8 (&out)[NS][NT / 2], int lane) {
  const int g = lane >> 4;
  f32x4 prev[NS];
#if NERF_BF16_IGLP >= 0
  __builtin_amdgcn_iglp_opt(NERF_BF16_IGLP);
#endif
  // epilogue of a finished tile, run under the next tile's MFMAs.  The empty asm pins it there: without it hipcc
  // reads the accumulators right behind their last MFMA (s_nop 6 in both waves of the SIMD at once).  ReLU after
  // the bf16 rounding, as a packed 16-bit integer max on the bit patterns: one VALU op per two values.
  auto finish = [&](int nt, f32x4 (&a)[NS]) {
#pragma unroll
    for (int s = 0; s < NS; ++s) asm volatile("" : "+v"(a[s]));
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int i = 0; i < 4; i += 2) {
        const bf16x2 pr = RELU ? relu_pack(a[s][i], a[s][i + 1]) : pack2(a[s][i], a[s][i + 1]);
        out[s][nt >> 1][4 * (nt & 1) + i] = pr[0];
        out[s][nt >> 1][4 * (nt & 1) + i + 1] = pr[1];
      }
  };
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const float4 b = ws.bias4(bias_slot + 16 * nt + 4 * g);
    f32x4 acc[NS];
    acc[0][0] = b.x; acc[0][1] = b.y; acc[0][2] = b.z; acc[0][3] = b.w;
#pragma unroll
    for (int s = 1; s < NS; ++s) acc[s] = acc[0];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const bf16x8 a = next_frag(ws, fbase + nt * KS + ks, lane);
      if (nt > 0 && ks == KS / 2) finish(nt - 1, prev);      // previous tile's epilogue, half a tile of MFMAs later
#pragma unroll
      for (int s = 0; s < NS; ++s) acc[s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, in[s][ks], acc[s], 0, 0, 0);
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) prev[s] = acc[s];
  }
  finish(NT - 1, prev);
}

// one wave: NS x 16 samples starting at sample wtile0 * 16 NS, encoded at the head of the pass (the pass queue is asked before the
// input loads).  Computing the NEXT pass's encodings behind the MFMAs of pos6 / pos7 instead was measured and gained nothing
// (DESIGN_HISTORY.md, profiles/r02_pe_hoist_ab.log).
template <int NS, class WS>
__device__ __forceinline__ void fwd_tiles16(const FwdArgs& a, WS& ws, int64_t wtile0, int64_t nwtiles, int lane, PassQueue& pq) {
  const int c = lane & 15, g = lane >> 4;
  bf16x8 pe[NS][2], dpe[NS][1];
  pq.ask(ws.wv, lane);                                  // before this pass's input loads
  {
    const GroupFreq q = group_freqs(a.fr, g);
    const int64_t wt = wtile0 < nwtiles ? wtile0 : nwtiles - 1;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const Sample sm = load_sample(a.rays, a.z, clamp_sample(wt * (16 * NS) + 16 * s + c, a.M), a.n);
#if NERF_ABLATE == 3          // timing-only build 3: no positional-encoding arithmetic
      bf16x8 cst;
      for (int j = 0; j < 8; ++j) cst[j] = (__bf16)(sm.p[0] + sm.d[0]);
      pe[s][0] = cst; pe[s][1] = cst; dpe[s][0] = cst;
#else
      encode_group<SinRevFract, PackBf16, false>(q, sm.p, pe[s]);
      encode_group<SinRevFract, PackBf16, true>(q, sm.d, dpe[s]);
#endif
    }
  }
  pq.publish(ws.wv);
  int bad[NS];                      // non-finite inputs of this lane's samples (mlp_frag.h: nonfinite_flags), used at the output store
#pragma unroll
  for (int s = 0; s < NS; ++s)
  {
    bad[s] = nonfinite_flags<16 | 32>(nonfinite_bits(pe[s][0]) | nonfinite_bits(pe[s][1]), nonfinite_bits(dpe[s][0]));
    asm volatile("" : "+v"(bad[s]));          // at the head of the pass (see fwd_tiles)
  }
  bf16x8 ha[NS][8], hb[NS][8];
  layer_fwd16<NS, 2, 16, true>(ws, L16::F_L0, 0, pe, ha, lane);
  layer_fwd16<NS, 8, 16, true>(ws, L16::F_L1 + 0 * 128, 256, ha, hb, lane);
  layer_fwd16<NS, 8, 16, true>(ws, L16::F_L1 + 1 * 128, 512, hb, ha, lane);
  layer_fwd16<NS, 8, 16, true>(ws, L16::F_L1 + 2 * 128, 768, ha, hb, lane);
  layer_fwd16<NS, 8, 16, true>(ws, L16::F_L1 + 3 * 128, 1024, hb, ha, lane);
  {
    bf16x8 cat[NS][10];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      cat[s][0] = pe[s][0]; cat[s][1] = pe[s][1];
#pragma unroll
      for (int k = 0; k < 8; ++k) cat[s][2 + k] = ha[s][k];
    }
    layer_fwd16<NS, 10, 16, true>(ws, L16::F_L5, 1280, cat, hb, lane);
  }
  layer_fwd16<NS, 8, 16, true>(ws, L16::F_L6, 1536, hb, ha, lane);
  layer_fwd16<NS, 8, 16, true>(ws, L16::F_L7, 1792, ha, hb, lane);
  layer_fwd16<NS, 8, 16, false>(ws, L16::F_FA, L::BI_FEAT, hb, ha, lane);
  float alpha[NS];
  {
    const float4 b = ws.bias4(L::BI_ALPHA + 4 * g);
    f32x4 acc[NS];
    acc[0][0] = b.x; acc[0][1] = b.y; acc[0][2] = b.z; acc[0][3] = b.w;
#pragma unroll
    for (int s = 1; s < NS; ++s) acc[s] = acc[0];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const bf16x8 wa = next_frag(ws, L16::F_FA + 128 + ks, lane);
#pragma unroll
      for (int s = 0; s < NS; ++s) acc[s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa, hb[s][ks], acc[s], 0, 0, 0);
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) alpha[s] = acc[s][0];
  }
  bf16x8 hd[NS][4];
  {
    bf16x8 cat[NS][9];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
#pragma unroll
      for (int k = 0; k < 8; ++k) cat[s][k] = ha[s][k];
      cat[s][8] = dpe[s][0];
    }
    layer_fwd16<NS, 9, 8, true>(ws, L16::F_DIR, L::BI_DIR, cat, hd, lane);
  }
  {
    const float4 b = ws.bias4(L::BI_RGB + 4 * g);
    f32x4 acc[NS];
    acc[0][0] = b.x; acc[0][1] = b.y; acc[0][2] = b.z; acc[0][3] = b.w;
#pragma unroll
    for (int s = 1; s < NS; ++s) acc[s] = acc[0];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const bf16x8 wr = next_frag(ws, L16::F_RGB + ks, lane);
#pragma unroll
      for (int s = 0; s < NS; ++s) acc[s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wr, hd[s][ks], acc[s], 0, 0, 0);
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int64_t m = wtile0 * (16 * NS) + 16 * s + c;
      if (g == 0 && wtile0 < nwtiles && m < a.M) {
        float4 o; o.x = acc[s][0]; o.y = acc[s][1]; o.z = acc[s][2]; o.w = alpha[s];
        *reinterpret_cast<float4*>(a.out + m * 4) = poison_raw(o, bad[s]);
      }
    }
  }
}

// NW waves x NS sample tiles of 16 = 256 samples per workgroup pass either way: <8, 2> two waves per SIMD at 256
// registers each; <4, 4> one wave per SIMD with the whole 512-register file, half the LDS fragment reads per FLOP.
template <int NW, int NS>
__global__ void __launch_bounds__(64 * NW) mlp_fwd_ring16_kernel(FwdArgs a) {
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t nwtiles = (a.M + 16 * NS - 1) / (16 * NS), nsuper = (nwtiles + NW - 1) / NW;
  NERF_STAMP2_DECL();
  RingW<L16::CHUNKS, L::F16_TOTAL, 4, NW> ws;
  ws.wsrc = reinterpret_cast<const char*>(a.wf);          // points at the 16x16x32 stream
  ws.lane16 = 16 * lane;
  ws.lds0 = __builtin_amdgcn_readfirstlane(lds_addr_of(ring_smem));
  ws.wv = wv;
  ws.start(lane);
  ring_load_bias(a.bias, L::BI_TOTAL);
  __syncthreads();
  NERF_STAMP_BEGIN();
  NERF_STAMP2_LOOP();
  PassQueue pq;                                         // dynamic pass queue (mlp_ring.h); a.queue == nullptr: static split
  pq.init(a.queue, ws.lds0 + RING_BIAS_OFF);
  for (int64_t sp = blockIdx.x; sp < nsuper;) {
    int ln = lane;
    asm volatile("" : "+v"(ln));
    ws.new_pass();
    fwd_tiles16<NS>(a, ws, sp * NW + wv, nwtiles, ln, pq);
    NERF_STAMP_PASS();
    NERF_STAMP2_PASS();
    sp = pq.next(sp);
  }
  NERF_STAMP_END();
  NERF_STAMP2_END();
  ws.drain();
  pq.leave();
}

// ------------------------------------------------------------------------------------------
// backward chain: dZ_l for every layer (stored as fragment blocks for the dW kernel)
// ------------------------------------------------------------------------------------------
// backward epilogue quarter: ReLU' from the forward's sign bits, then bf16
template <bool MASK, int Q, int ODD>
__device__ __forceinline__ void finish_quarter_bwd_t(const f32x16& acc, bf16x8& lo, bf16x8& hi, unsigned w) {
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int i = 4 * Q + 2 * p;
    bf16x2 pr = pack2(acc[i], acc[i + 1]);
    if (MASK) pr = p == 0 ? keep_where<8 * ODD + 2 * Q>(pr, w) : keep_where<8 * ODD + 2 * Q + 1>(pr, w);
    if (i < 8) { lo[i] = pr[0]; lo[i + 1] = pr[1]; } else { hi[i - 8] = pr[0]; hi[i - 7] = pr[1]; }
  }
}
template <bool MASK>
__device__ __forceinline__ void finish_quarter_bwd(const f32x16& acc, int q, int kt, bf16x8& lo, bf16x8& hi,
                                                   const u32x4& mask) {
  const unsigned w = MASK ? mask[kt >> 1] : 0u;
  // q and kt are compile-time constants at every call site (fully unrolled loops): the switch folds away
  switch (2 * q + (kt & 1)) {
    case 0: finish_quarter_bwd_t<MASK, 0, 0>(acc, lo, hi, w); break;
    case 1: finish_quarter_bwd_t<MASK, 0, 1>(acc, lo, hi, w); break;
    case 2: finish_quarter_bwd_t<MASK, 1, 0>(acc, lo, hi, w); break;
    case 3: finish_quarter_bwd_t<MASK, 1, 1>(acc, lo, hi, w); break;
    case 4: finish_quarter_bwd_t<MASK, 2, 0>(acc, lo, hi, w); break;
    case 5: finish_quarter_bwd_t<MASK, 2, 1>(acc, lo, hi, w); break;
    case 6: finish_quarter_bwd_t<MASK, 3, 0>(acc, lo, hi, w); break;
    default: finish_quarter_bwd_t<MASK, 3, 1>(acc, lo, hi, w); break;
  }
}

// out[t][2 kt + s] = mask( W^T[kt-tile] . in[t] );  mask = ReLU sign bits written by the forward kernel
template <int ST, int NS, int KT, bool MASK, class WS, class SINK = NoSink>
__device__ __forceinline__ void layer_bwd(WS& ws, int fbase, const bf16x8 (&in)[ST][NS], bf16x8 (&out)[ST][2 * KT],
                                          const u32x4 (&mask)[ST], int lane, const SINK& sink = SINK()) {
  f32x16 prev[ST];
#pragma unroll
  for (int kt = 0; kt < KT; ++kt) {
    f32x16 acc[ST];
#pragma unroll
    for (int t = 0; t < ST; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;
#pragma unroll
    for (int ns = 0; ns < NS; ++ns) {
      const bf16x8 a = next_frag(ws, fbase + kt * NS + ns, lane);
#pragma unroll
      for (int t = 0; t < ST; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, in[t][ns], acc[t], 0, 0, 0);
      if (kt > 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (quarter_pos(NS, q) == ns) {
#pragma unroll
            for (int t = 0; t < ST; ++t) {
              finish_quarter_bwd<MASK>(prev[t], q, kt - 1, out[t][2 * kt - 2], out[t][2 * kt - 1], mask[t]);
              if (q == 3) { sink.put(t, 2 * kt - 2, out[t][2 * kt - 2]); sink.put(t, 2 * kt - 1, out[t][2 * kt - 1]); }
            }
          }
      }
    }
#pragma unroll
    for (int t = 0; t < ST; ++t) prev[t] = acc[t];
  }
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int t = 0; t < ST; ++t)
      finish_quarter_bwd<MASK>(prev[t], q, KT - 1, out[t][2 * KT - 2], out[t][2 * KT - 1], mask[t]);
#pragma unroll
  for (int t = 0; t < ST; ++t) { sink.put(t, 2 * KT - 2, out[t][2 * KT - 2]); sink.put(t, 2 * KT - 1, out[t][2 * KT - 1]); }
}

struct BwdArgs {
  unsigned* queue;       // dynamic pass queue slot of this launch, or nullptr (static split): mlp_ring.h
  const bf16x8* wb;
  const void* acts;
  const float* d_raw;    // [M,4]
  int64_t M;
  void* dz;
  int64_t astride, zstride;
};

template <int ST, class WS>
__device__ __forceinline__ void bwd_tiles(const BwdArgs& a, WS& ws, int64_t tile0, int64_t ntiles, int lane, PassQueue* pq = nullptr) {
  const int r = lane & 31, h = lane >> 5;
  if (pq) pq->ask(ws_wave(ws), lane);          // dynamic pass queue (mlp_ring.h): before this pass's input loads
  int64_t tile[ST];
  bool live[ST];
  bf16x8 zrgb[ST][1], zal[ST][1];
#pragma unroll
  for (int t = 0; t < ST; ++t) {
    live[t] = tile0 + t < ntiles;
    tile[t] = live[t] ? tile0 + t : ntiles - 1;
    const int64_t m = tile[t] * 32 + r;
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live[t] && m < a.M && h == 0) g = *reinterpret_cast<const float4*>(a.d_raw + m * 4);
#pragma unroll
    for (int j = 0; j < 8; ++j) { zrgb[t][0][j] = (__bf16)0.0f; zal[t][0][j] = (__bf16)0.0f; }
    zrgb[t][0][0] = (__bf16)g.x; zrgb[t][0][1] = (__bf16)g.y; zrgb[t][0][2] = (__bf16)g.z;   // rows 0..2 (h == 0)
    zal[t][0][0] = (__bf16)g.w;                                                              // row 0
  }
  if (pq) pq->publish(ws_wave(ws));
  // every ReLU mask of the pass is fetched here, so the chain itself issues no loads the compiler must wait for
  u32x4 mk[9][ST];
#pragma unroll
  for (int l = 0; l < 9; ++l)
#pragma unroll
    for (int t = 0; t < ST; ++t)
      mk[l][t] = *reinterpret_cast<const u32x4*>(frag_ptr(const_cast<void*>(a.acts), tile[t], a.astride, L::A_MASK + l, r, h));
#define store(slot0, t, frags, count) \
  do { store_frags<count>(a.dz, tile0 + (t), a.zstride, slot0, frags, r, h); ws.note_stores(count); } while (0)
#pragma unroll
  for (int t = 0; t < ST; ++t) { store(L::Z_RGB, t, zrgb[t], 1); store(L::Z_A, t, zal[t], 1); }

#define ZSINK(slot0) FragSink<true>{a.dz, tile0, a.zstride, slot0, r, h}
  bf16x8 zd[ST][8];
  layer_bwd<ST, 1, 4, true>(ws, L::B_RGB, zrgb, zd, mk[8], lane, ZSINK(L::Z_D));
  bf16x8 za[ST][16], zb[ST][16];
  layer_bwd<ST, 8, 8, false>(ws, L::B_DIR, zd, za, mk[8], lane, ZSINK(L::Z_F));            // d feature
  {
    bf16x8 cat[ST][17];
#pragma unroll
    for (int t = 0; t < ST; ++t) {
#pragma unroll
      for (int k = 0; k < 16; ++k) cat[t][k] = za[t][k];
      cat[t][16] = zal[t][0];
    }
    layer_bwd<ST, 17, 8, true>(ws, L::B_FA, cat, zb, mk[7], lane, ZSINK(L::Z_L0 + 112));   // dZ7
  }
  layer_bwd<ST, 16, 8, true>(ws, L::B_L7, zb, za, mk[6], lane, ZSINK(L::Z_L0 + 96));       // dZ6
  layer_bwd<ST, 16, 8, true>(ws, L::B_L6, za, zb, mk[5], lane, ZSINK(L::Z_L0 + 80));       // dZ5
  layer_bwd<ST, 16, 8, true>(ws, L::B_L5, zb, za, mk[4], lane, ZSINK(L::Z_L0 + 64));       // dZ4
  layer_bwd<ST, 16, 8, true>(ws, L::B_L4 + 0 * 128, za, zb, mk[3], lane, ZSINK(L::Z_L0 + 48));   // dZ3
  layer_bwd<ST, 16, 8, true>(ws, L::B_L4 + 1 * 128, zb, za, mk[2], lane, ZSINK(L::Z_L0 + 32));   // dZ2
  layer_bwd<ST, 16, 8, true>(ws, L::B_L4 + 2 * 128, za, zb, mk[1], lane, ZSINK(L::Z_L0 + 16));   // dZ1
  layer_bwd<ST, 16, 8, true>(ws, L::B_L4 + 3 * 128, zb, za, mk[0], lane, ZSINK(L::Z_L0 + 0));    // dZ0
#undef store
#undef ZSINK
}

template <int ST>
__global__ void __launch_bounds__(256, (ST == 1 ? 2 : 1)) mlp_bwd_kernel(BwdArgs a) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t tile0 = ((int64_t)blockIdx.x * 4 + wv) * ST;
  const int64_t ntiles = (a.M + 31) >> 5;
  if (tile0 >= ntiles) return;
  GlobalW ws{a.wb + lane, nullptr};
  bwd_tiles<ST>(a, ws, tile0, ntiles, lane);
}

// the transposed stream is padded with zero fragments to whole chunks (1100 -> 1120 = 35 x 32 = 70 x 16)
template <int NW = 8, int CHUNK = RING_CHUNK>
__global__ void __launch_bounds__(64 * NW, 2) mlp_bwd_ring_kernel(BwdArgs a) {
  static_assert(L::B_PADDED % CHUNK == 0, "padded backward stream must be whole chunks");
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t ntiles = (a.M + 31) >> 5;
  const int64_t nsuper = (ntiles + NW - 1) / NW;
  RingW<(L::B_TOTAL + CHUNK - 1) / CHUNK, L::B_TOTAL, 4, NW, CHUNK> ws;
  ws.wsrc = reinterpret_cast<const char*>(a.wb);
  ws.lane16 = 16 * lane;
  ws.lds0 = __builtin_amdgcn_readfirstlane(lds_addr_of(ring_smem));
  ws.wv = wv;
  ws.start(lane);
  PassQueue pq;                                         // dynamic pass queue (mlp_ring.h); a.queue == nullptr: static split
  pq.init(a.queue, ws.lds0 + decltype(ws)::BIAS_OFF);
  for (int64_t sp = blockIdx.x; sp < nsuper;) {
    int ln = lane;
    asm volatile("" : "+v"(ln));
    ws.new_pass();
    bwd_tiles<1>(a, ws, sp * NW + wv, ntiles, ln, &pq);
    // the pass ends inside the last chunk (1100 is not a multiple of the chunk): nothing else to do, the next pass starts
    // at a chunk boundary again because fragment indices restart at 0
    sp = pq.next(sp);
  }
  ws.drain();
  pq.leave();
}

// ------------------------------------------------------------------------------------------
// dW: split-K GEMMs  dW[n][k] = sum_m dZ[n][m] H[k][m]  over fragment blocks, samples = MFMA K
// ------------------------------------------------------------------------------------------

constexpr int DW_FRAG_STRIDE = 1152;                 // 1 KiB + 128 B: neighbouring fragments hit disjoint banks
constexpr int DW_STAGE_BYTES = 32 * DW_FRAG_STRIDE;  // 16 dZ + 16 act fragments per 32-sample tile
constexpr int DW_STAGES = 4;                         // LDS-DMA ring: 3 tiles in flight behind the one being consumed
constexpr int DW_LDS_BYTES = DW_STAGES * DW_STAGE_BYTES + 1024;   // + 1 KiB sink for padding DMAs

__device__ __forceinline__ bf16x8 tr_frag(const char* lds_frag, int u, int hq, int i16) {
  // A/B operand of v_mfma_f32_32x32x16_bf16 with K = samples 16u + 8hq + (0..7) and row/col = feature (natural
  // order).  Lane i16 = 4q + p of a 16-lane group addresses sample row q, feature piece p (h_src = p&1, j half = p>>1).
  const int q = i16 >> 2, p = i16 & 3;
  const char* base = lds_frag + 16 * (p & 1) + 8 * (p >> 1) + 32 * (16 * u + 8 * hq + q);
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(base));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(base + 128));
  union { struct { s16x4 a, b; } s; bf16x8 v; } cvt;
  cvt.s.a = lo; cvt.s.b = hi;
  return cvt.v;
}

#ifndef NERF_DW_WAVES
#define NERF_DW_WAVES 16
#endif
constexpr int DW_WAVES = NERF_DW_WAVES;          // 8: 4 x 2 output tiles per wave; 16: 2 x 2 (half the accumulators, 4 waves per SIMD)
constexpr int DW_NPW = 32 / DW_WAVES;            // n-tiles per wave = DMAs per wave per tile
__global__ void __launch_bounds__(64 * DW_WAVES) mlp_dw_kernel(DwArgs a) {
  char* smem = ring_smem;                             // the one dynamic-LDS array of this file
  int bj = blockIdx.x, job_id = 0;
  while (bj >= a.splits[job_id]) { bj -= a.splits[job_id]; ++job_id; }
  const DwJob jb = a.jobs[job_id];
  const int tile_lo = (int)((int64_t)a.ntiles * bj / a.splits[job_id]);
  const int tile_hi = (int)((int64_t)a.ntiles * (bj + 1) / a.splits[job_id]);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n_tiles = (jb.nf + 1) >> 1, k_tiles = (jb.kf + 1) >> 1;
  // wave (wr, wc) of the 4 x 4 wave grid.  A wave runs on SIMD wv % 4: with wr = wv / 4 the waves of one wave COLUMN share a SIMD,
  // and a job with k_tiles <= 2 (pos0, pos5 | PE, dir0 | dirPE: only column 0 has work) puts all its MFMAs on SIMD 0 while three
  // SIMDs idle.  Such jobs use the transposed numbering (round 5): their active waves are wv = 0..3, one per SIMD.
  const bool col_major = DW_WAVES == 16 && k_tiles <= 2;
  const int wr = col_major ? (wv & 3) : (wv >> 2), wc = col_major ? (wv >> 2) : (wv & 3);
  const int nf_pad = n_tiles * 2;
  const int nfk = jb.nf + jb.kf;                        // real fragments per sample tile (<= 32)
  // this wave's output tiles: n-tiles wr*DW_NPW + (0..DW_NPW-1), k-tiles wc*2 + (0..1)
  const bool active = (wr * DW_NPW < n_tiles) && (wc * 2 < k_tiles);
  f32x16 acc[DW_NPW][2];
#pragma unroll
  for (int i = 0; i < DW_NPW; ++i)
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][k][e] = 0.0f;
  float bsum[DW_NPW];
#pragma unroll
  for (int i = 0; i < DW_NPW; ++i) bsum[i] = 0.0f;
  const int g16 = lane >> 4, i16 = lane & 15, hq = g16 >> 1, fsel = g16 & 1;
  const bf16x8* dzp = reinterpret_cast<const bf16x8*>(a.dz) + lane;
  const bf16x8* acp = reinterpret_cast<const bf16x8*>(a.acts) + lane;
  const unsigned lds0 = __builtin_amdgcn_readfirstlane(lds_addr_of(smem));
  const unsigned sink = lds0 + DW_STAGES * DW_STAGE_BYTES;

  // odd fragment counts (rgb / alpha jobs: nf = 1): the partner fragment of the tile is never written by DMA
  if (jb.nf & 1) {
    for (int c = tid; c < DW_STAGES * 64; c += 64 * DW_WAVES) {
      bf16x8 zv;
#pragma unroll
      for (int j = 0; j < 8; ++j) zv[j] = (__bf16)0.0f;
      *reinterpret_cast<bf16x8*>(smem + (c >> 6) * DW_STAGE_BYTES + jb.nf * DW_FRAG_STRIDE + (c & 63) * 16) = zv;
    }
  }
  // every wave issues exactly DW_NPW DMAs per tile so that vmcnt arithmetic is uniform: fragment ids wv + DW_WAVES k
  auto issue = [&](int tile, int stage) {
    const unsigned st = lds0 + __builtin_amdgcn_readfirstlane(stage) * DW_STAGE_BYTES;
#pragma unroll
    for (int k = 0; k < DW_NPW; ++k) {
      const int i = wv + DW_WAVES * k;
      if (i < jb.nf) dma_frag_nt(dzp + (int64_t)tile * a.zstride + (jb.dz_slot + i) * 64, st + i * DW_FRAG_STRIDE);
      else if (i < nfk) dma_frag_nt(acp + (int64_t)tile * a.astride + (jb.act_slot + (i - jb.nf)) * 64,
                                 st + (nf_pad + i - jb.nf) * DW_FRAG_STRIDE);
      else dma_frag(dzp + (int64_t)tile * a.zstride + jb.dz_slot * 64, sink);      // padding: L2 hit, result unused
    }
  };
  __syncthreads();                                      // zero fill visible before any stage is consumed
#pragma unroll
  for (int s_ = 0; s_ < DW_STAGES - 1; ++s_)
    if (tile_lo + s_ < tile_hi) issue(tile_lo + s_, s_);

  for (int tile = tile_lo; tile < tile_hi; ++tile) {
    const int rem = tile_hi - 1 - tile;                 // tiles issued after this one and still in flight (<= 2)
    // lgkmcnt(0): this wave's transposed reads of the previous tile are complete before the barrier lets another
    // wave's DMA refill that stage (hipcc may sink register-only MFMAs, and their waits, below an asm statement)
    if (DW_NPW == 4) {
      if (rem >= 2) asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" ::: "memory");
      else if (rem == 1) asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    } else {
      if (rem >= 2) asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
      else if (rem == 1) asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();                       // tile landed for every wave; stage (tile-1)%4 is free
    if (tile + DW_STAGES - 1 < tile_hi) issue(tile + DW_STAGES - 1, (tile - tile_lo + DW_STAGES - 1) % DW_STAGES);
    const char* st = smem + ((tile - tile_lo) % DW_STAGES) * DW_STAGE_BYTES;
#if NERF_ABLATE == 4          // timing-only: loads and synchronisation only
    if (false) {
#else
    if (active) {
#endif
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        bf16x8 bfr[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const int kt = wc * 2 + k;
          const int f = nf_pad + (kt < k_tiles ? 2 * kt : 0) + fsel;
          bfr[k] = tr_frag(st + f * DW_FRAG_STRIDE, u, hq, i16);
        }
#pragma unroll
        for (int i = 0; i < DW_NPW; ++i) {
          const int nt = wr * DW_NPW + i;
          const int f = (nt < n_tiles ? 2 * nt : 0) + fsel;
          const bf16x8 afr = tr_frag(st + f * DW_FRAG_STRIDE, u, hq, i16);
#if NERF_ABLATE != 5          // timing-only build 5: no bias row sums
          if (wc == 0) {                       // bias gradient = row sums of dZ: v_dot2c_f32_bf16 against (1, 1)
            typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
            const bf16x2_t ones = {(__bf16)1.0f, (__bf16)1.0f};
#pragma unroll
            for (int j = 0; j < 8; j += 2) {
              const bf16x2_t pr = {afr[j], afr[j + 1]};
              bsum[i] = __builtin_amdgcn_fdot2_f32_bf16(pr, ones, bsum[i], false);
            }
          }
#endif
#pragma unroll
          for (int k = 0; k < 2; ++k) acc[i][k] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(afr, bfr[k], acc[i][k], 0, 0, 0);
        }
      }
    }
  }
  if (!active) return;
#if NERF_ABLATE == 6          // timing-only build 6: no epilogue
  if (a.ntiles > 0) return;
#endif
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
      const float tot = bsum[i] + __shfl_xor(bsum[i], 32, 64);      // the two sample halves of the k-step
      if (hh == 0) slot[64 * 1024 + 32 * nt + rr] = tot;
    }
  }
}

// grads[w_off + n ldw + col0 + k] = sum over the job's splits of its partial tiles, in split order (deterministic);
// blockIdx.y = job, one thread per output element (weights first, then the bias row of jobs that own one).  The S loads
// of an element are independent (issued eight at a time), only the adds are a chain.
__global__ void __launch_bounds__(256) mlp_dw_reduce_kernel(DwArgs a) {
  const int j = blockIdx.y;
  const DwJob jb = a.jobs[j];
  int first = 0;
  for (int q = 0; q < j; ++q) first += a.splits[q];
  const int S = a.splits[j];
  const int nw = jb.n_valid * jb.k_valid, nb = jb.b_off >= 0 ? jb.n_valid : 0;
  const float* base = a.partial + (size_t)first * DW_SLOT_FLOATS;
  for (int t = blockIdx.x * 256 + threadIdx.x; t < nw + nb; t += gridDim.x * 256) {
    const float* src;
    float* dst;
    if (t < nw) {
      const int n = t / jb.k_valid, k = t - n * jb.k_valid;
      src = base + (8 * (n >> 5) + (k >> 5)) * 1024 + (n & 31) * 32 + (k & 31);
      dst = a.grads + jb.w_off + (int64_t)n * jb.ldw + jb.col0 + k;
      if (jb.aux_row0 > 0) {                   // (DwJob) rows that are no gradient: to aux, or nowhere
        if (n >= jb.aux_row0) dst = a.aux + (n - jb.aux_row0) * jb.k_valid + k;
        else if (n >= jb.n_grad) continue;
      }
    } else {
      const int n = t - nw;
      src = base + 64 * 1024 + n;
      dst = a.grads + jb.b_off + n;
      if (jb.aux_row0 > 0) {
        if (n >= jb.aux_row0) dst = a.aux + (jb.n_valid - jb.aux_row0) * jb.k_valid + (n - jb.aux_row0);
        else if (n >= jb.n_grad) continue;
      }
    }
    float sum = 0.0f;
    int sidx = 0;
    for (; sidx + 8 <= S; sidx += 8) {
      float v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = __builtin_nontemporal_load(src + (size_t)(sidx + q) * DW_SLOT_FLOATS);
#pragma unroll
      for (int q = 0; q < 8; ++q) sum += v[q];
    }
    for (; sidx < S; ++sidx) sum += __builtin_nontemporal_load(src + (size_t)sidx * DW_SLOT_FLOATS);
    *dst = sum;
  }
}


// ==========================================================================================
// Second architecture: the no-view-direction model of the reference's 2-D image fitting
// (entrypoints/__viser_image_learning.py:198-208: NeRF(channel_input=40, channel_input_views=0, channel_output=3,
// is_use_view_directions=False)): pos0 [256x40] pos1..4 [256x256] pos5 [256x296] pos6 pos7 output [out_ch x 256]
// (models/NeRF.py:182-197,241).  Same register-resident transposed scheme, same ring, same dW kernel.
// ==========================================================================================

// index maps and pack description (ImgPack): mlp_arch2.h; ImgArgs: mlp_input2.h
static_assert(LI::F_CHUNKS * RING_CHUNK == LI::F_TOTAL && LI::B_CHUNKS * RING_CHUNK == LI::B_PADDED, "whole ring chunks");

template <bool STORE, class WS>
__device__ __forceinline__ void fwd_tiles_img(const ImgArgs& a, WS& ws, int64_t tile0, int64_t ntiles, int lane) {
  constexpr int ST = 1;
  const int r = lane & 31, h = lane >> 5;
  int64_t tile = tile0 < ntiles ? tile0 : ntiles - 1;
  int64_t m = tile * 32 + r; if (m >= a.M) m = a.M - 1;
  bf16x8 xin[ST][3];
#pragma unroll
  for (int ks = 0; ks < 3; ++ks) row_pairs<CvtBf16>(a.x + m * LI::CIN, ks, h, LI::CIN, xin[0][ks]);
  int bad = nonfinite_flags<32>(nonfinite_bits(xin[0][0]) | nonfinite_bits(xin[0][1]) | nonfinite_bits(xin[0][2]), 0u);
  asm volatile("" : "+v"(bad));               // at the head of the pass (see fwd_tiles)
  if (STORE) { store_frags<3>(a.acts, tile0, a.astride, LI::A_X, xin[0], r, h); ws.note_stores(3); }
  bf16x8 ha[ST][16], hb[ST][16];
  u32x4 mk[ST];
#define IMG_LAYER(KS, FB, BS, IN, OUT, LYR)                                                        \
  do { mk[0] = u32x4{0u, 0u, 0u, 0u};                                                              \
       layer_fwd<ST, KS, 8, true, STORE>(ws, FB, BS, IN, OUT, mk, lane);                           \
       if (STORE) { store_frags<16>(a.acts, tile0, a.astride, LI::A_H0 + 16 * (LYR), OUT[0], r, h); \
                    *reinterpret_cast<u32x4*>(frag_ptr(a.acts, tile0, a.astride, LI::A_MASK + (LYR), r, h)) = mk[0]; ws.note_stores(17); } } while (0)
  IMG_LAYER(3, LI::F_L0, 0, xin, ha, 0);
  IMG_LAYER(16, LI::F_L1 + 0 * 128, 256, ha, hb, 1);
  IMG_LAYER(16, LI::F_L1 + 1 * 128, 512, hb, ha, 2);
  IMG_LAYER(16, LI::F_L1 + 2 * 128, 768, ha, hb, 3);
  IMG_LAYER(16, LI::F_L1 + 3 * 128, 1024, hb, ha, 4);
  {
    bf16x8 cat[ST][19];
    if (STORE) {
#pragma unroll
      for (int k = 0; k < 3; ++k) xin[0][k] = *frag_ptr(a.acts, tile0, a.astride, LI::A_X + k, r, h);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) cat[0][k] = xin[0][k];
#pragma unroll
    for (int k = 0; k < 16; ++k) cat[0][3 + k] = ha[0][k];
    IMG_LAYER(19, LI::F_L5, 1280, cat, hb, 5);           // concat [input_pos, h]  models/NeRF.py:224-225
  }
  IMG_LAYER(16, LI::F_L6, 1536, hb, ha, 6);
  IMG_LAYER(16, LI::F_L7, 1792, ha, hb, 7);
#undef IMG_LAYER
  f32x16 acc;
  acc_init_bias(acc, ws, LI::BI_OUT, h);
#pragma unroll
  for (int ks = 0; ks < 16; ++ks) {
    const bf16x8 wo = next_frag(ws, LI::F_OUT + ks, lane);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wo, hb[0][ks], acc, 0, 0, 0);
  }
  const int64_t mo = tile0 * 32 + r;
  if (h == 0 && tile0 < ntiles && mo < a.M) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < a.out_ch) a.out[mo * a.out_ch + c] = bad ? __builtin_nanf("") : acc[c];      // output_linear (models/NeRF.py:241); NaN / Inf inputs: mlp_frag.h
  }
}

template <bool STORE>
__global__ void __launch_bounds__(512, 2) mlp_img_fwd_ring_kernel(ImgArgs a) {
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t ntiles = (a.M + 31) >> 5, nsuper = (ntiles + 7) >> 3;
  RingW<LI::F_CHUNKS, LI::F_TOTAL, (STORE ? 2 : 4)> ws;
  ws.wsrc = reinterpret_cast<const char*>(a.wf);
  ws.lane16 = 16 * lane;
  ws.lds0 = __builtin_amdgcn_readfirstlane(lds_addr_of(ring_smem));
  ws.wv = wv;
  ws.start(lane);
  ring_load_bias(a.bias, LI::BI_TOTAL);
  __syncthreads();
  for (int64_t sp = blockIdx.x; sp < nsuper; sp += gridDim.x) {
    int ln = lane;
    asm volatile("" : "+v"(ln));
    ws.new_pass();
    fwd_tiles_img<STORE>(a, ws, sp * 8 + wv, ntiles, ln);
  }
  ws.drain();
}

__global__ void __launch_bounds__(512, 2) mlp_img_bwd_ring_kernel(ImgArgs a) {
  constexpr int ST = 1;
  const int lane0 = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t ntiles = (a.M + 31) >> 5, nsuper = (ntiles + 7) >> 3;
  RingW<LI::B_CHUNKS, LI::B_TOTAL> ws;
  ws.wsrc = reinterpret_cast<const char*>(a.wb);
  ws.lane16 = 16 * lane0;
  ws.lds0 = __builtin_amdgcn_readfirstlane(lds_addr_of(ring_smem));
  ws.wv = wv;
  ws.start(lane0);
  for (int64_t sp = blockIdx.x; sp < nsuper; sp += gridDim.x) {
    int lane = lane0;
    asm volatile("" : "+v"(lane));
    ws.new_pass();
    const int r = lane & 31, h = lane >> 5;
    const int64_t tile0 = sp * 8 + wv;
    const int64_t tile = tile0 < ntiles ? tile0 : ntiles - 1;
    const int64_t m = tile * 32 + r;
    bf16x8 zo[ST][1];
#pragma unroll
    for (int j = 0; j < 8; ++j) zo[0][0][j] = (__bf16)0.0f;
    if (tile0 < ntiles && m < a.M && h == 0) {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < a.out_ch) zo[0][0][c] = (__bf16)a.d_out[m * a.out_ch + c];      // rows 0..out_ch-1
    }
    u32x4 mk[8][ST];
#pragma unroll
    for (int l = 0; l < 8; ++l)
      mk[l][0] = *reinterpret_cast<const u32x4*>(frag_ptr(a.acts, tile, a.astride, LI::A_MASK + l, r, h));
    store_frags<1>(a.dz, tile0, a.zstride, LI::Z_OUT, zo[0], r, h); ws.note_stores(1);
    bf16x8 za[ST][16], zb[ST][16];
    layer_bwd<ST, 1, 8, true>(ws, LI::B_OUT, zo, zb, mk[7], lane);                                  // dZ7
    store_frags<16>(a.dz, tile0, a.zstride, LI::Z_L0 + 112, zb[0], r, h); ws.note_stores(16);
    layer_bwd<ST, 16, 8, true>(ws, LI::B_L7 + 0 * 128, zb, za, mk[6], lane);                        // dZ6
    store_frags<16>(a.dz, tile0, a.zstride, LI::Z_L0 + 96, za[0], r, h); ws.note_stores(16);
    layer_bwd<ST, 16, 8, true>(ws, LI::B_L7 + 1 * 128, za, zb, mk[5], lane);                        // dZ5
    store_frags<16>(a.dz, tile0, a.zstride, LI::Z_L0 + 80, zb[0], r, h); ws.note_stores(16);
    layer_bwd<ST, 16, 8, true>(ws, LI::B_L7 + 2 * 128, zb, za, mk[4], lane);                        // dZ4
    store_frags<16>(a.dz, tile0, a.zstride, LI::Z_L0 + 64, za[0], r, h); ws.note_stores(16);
    layer_bwd<ST, 16, 8, true>(ws, LI::B_L7 + 3 * 128, za, zb, mk[3], lane);                        // dZ3
    store_frags<16>(a.dz, tile0, a.zstride, LI::Z_L0 + 48, zb[0], r, h); ws.note_stores(16);
    layer_bwd<ST, 16, 8, true>(ws, LI::B_L7 + 4 * 128, zb, za, mk[2], lane);                        // dZ2
    store_frags<16>(a.dz, tile0, a.zstride, LI::Z_L0 + 32, za[0], r, h); ws.note_stores(16);
    layer_bwd<ST, 16, 8, true>(ws, LI::B_L7 + 5 * 128, za, zb, mk[1], lane);                        // dZ1
    store_frags<16>(a.dz, tile0, a.zstride, LI::Z_L0 + 16, zb[0], r, h); ws.note_stores(16);
    layer_bwd<ST, 16, 8, true>(ws, LI::B_L7 + 6 * 128, zb, za, mk[0], lane);                        // dZ0
    store_frags<16>(a.dz, tile0, a.zstride, LI::Z_L0 + 0, za[0], r, h); ws.note_stores(16);
  }
  ws.drain();
}


// ==========================================================================================
// Third architecture: the reference's NeRF class at Instant-NGP size (BASELINE configs[4]: hash-grid features +
// tiny MLP): NeRF(n_layers=2, width_layers=64, channel_input=32 [16 levels x 2 features], channel_input_views=16
// [SH degree 3], list_skip_connection_layers=[], is_use_view_directions=True)  (models/NeRF.py:160-243):
// pos0 [64x32] pos1 [64x64] feature [64x64] alpha [1x64] dir0 [32x80] rgb [3x32] = 13 188 parameters.
// All 31 forward (27 backward) fragments fit LDS, so there is no ring: every workgroup copies its stream once and
// its 8 waves then run independently over sample tiles.  Same register-resident chain, same fragment-block stores,
// same dW kernel (7 jobs); the chain additionally returns dL/d(input features) for the hash-grid backward.
// ==========================================================================================
// index maps and pack description (SmallPack): mlp_arch2.h

// weight source (3): the whole stream resident in LDS (copied once per workgroup)
struct LdsW {
  __device__ __forceinline__ bf16x8 frag(int f, int lane) { return *reinterpret_cast<const bf16x8*>(ring_smem + f * 1024 + lane * 16); }
  __device__ __forceinline__ void note_stores(int) {}
  __device__ __forceinline__ float4 bias4(int slot) { return *reinterpret_cast<const float4*>(ring_smem + 32 * 1024 + slot * 4); }
};
__device__ __forceinline__ void lds_load_stream(const bf16x8* __restrict__ w, const float* __restrict__ bias) {
  for (int i = threadIdx.x; i < 32 * 64; i += blockDim.x) *reinterpret_cast<bf16x8*>(ring_smem + i * 16) = w[i];
  if (bias)
    for (int i = threadIdx.x; i < LN::BI_TOTAL; i += blockDim.x) *reinterpret_cast<float*>(ring_smem + 32 * 1024 + 4 * i) = bias[i];
  __syncthreads();
}

// SmallArgs, the tile map and the fused row stage (ngp_row: B fragments straight from the hash tables): mlp_input2.h

template <bool STORE, bool FUSED, bool LW = false>
__global__ void __launch_bounds__(512) mlp_small_fwd_kernel(SmallArgs a) {
  constexpr int ST = 1;
  lds_load_stream(a.wf, a.bias);
  const int lane0 = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const bool rmaj = FUSED && !STORE && a.ray_major;
  const int64_t ntiles = rmaj ? ((a.B + 31) >> 5) * a.n : (a.M + 31) >> 5;
  LdsW ws;
  for (int64_t tile0 = (int64_t)blockIdx.x * 8 + wv; tile0 < ntiles; tile0 += (int64_t)gridDim.x * 8) {
    int lane = lane0;
    asm volatile("" : "+v"(lane));        // fragment addresses are per-tile values: the 31 LDS reads are not hoisted (spills)
    const int r = lane & 31, h = lane >> 5;
    const TileSample ts = small_tile_sample(a, tile0, r, rmaj);
    const int64_t m = ts.m;
    const bool valid = ts.valid;
    bf16x8 in[3];                          // position k-steps 0, 1 | direction
    if (FUSED) {
      if (a.tables_h) ngp_row<true, LW, CvtBf16>(a, m, h, in);        // wave-uniform
      else ngp_row<false, LW, CvtBf16>(a, m, h, in);
    } else {
      small_row<CvtBf16>(a.x + m * LN::CIN, h, in);
    }
    bf16x8 xin[ST][2], din[ST][1];
    xin[0][0] = in[0]; xin[0][1] = in[1]; din[0][0] = in[2];
    int bad = nonfinite_flags<32>(nonfinite_bits(xin[0][0]) | nonfinite_bits(xin[0][1]), nonfinite_bits(din[0][0]));
    asm volatile("" : "+v"(bad));         // at the head of the tile (see fwd_tiles)
#define SINK(slot0) FragSink<STORE>{a.acts, tile0, a.astride, slot0, r, h}
#define MASK_STORE(layer) do { if (STORE) *reinterpret_cast<u32x4*>(frag_ptr(a.acts, tile0, a.astride, LN::A_MASK + (layer), r, h)) = mk[0]; } while (0)
    if (STORE) { store_frags<2>(a.acts, tile0, a.astride, LN::A_X, xin[0], r, h); store_frags<1>(a.acts, tile0, a.astride, LN::A_DX, din[0], r, h); }
    u32x4 mk[ST];
    bf16x8 h0[ST][4], h1[ST][4], ft[ST][4];
    mk[0] = u32x4{0u, 0u, 0u, 0u};
    layer_fwd<ST, 2, 2, true, STORE>(ws, LN::F_L0, LN::BI_L0, xin, h0, mk, lane, SINK(LN::A_H0));
    MASK_STORE(0);
    mk[0] = u32x4{0u, 0u, 0u, 0u};
    layer_fwd<ST, 4, 2, true, STORE>(ws, LN::F_L1, LN::BI_L1, h0, h1, mk, lane, SINK(LN::A_H1));
    MASK_STORE(1);
    layer_fwd<ST, 4, 2, false, false>(ws, LN::F_FA, LN::BI_FEAT, h1, ft, mk, lane, SINK(LN::A_FEAT));
    float alpha;
    {
      f32x16 acc;
      acc_init_bias(acc, ws, LN::BI_ALPHA, h);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ws.frag(LN::F_FA + 8 + ks, lane), h1[0][ks], acc, 0, 0, 0);
      alpha = acc[0];
    }
    bf16x8 hd[ST][2];
    {
      bf16x8 cat[ST][5];
#pragma unroll
      for (int k = 0; k < 4; ++k) cat[0][k] = ft[0][k];
      cat[0][4] = din[0][0];
      mk[0] = u32x4{0u, 0u, 0u, 0u};
      layer_fwd<ST, 5, 1, true, STORE>(ws, LN::F_DIR, LN::BI_DIR, cat, hd, mk, lane, SINK(LN::A_HD));
      MASK_STORE(2);
    }
    {
      f32x16 acc;
      acc_init_bias(acc, ws, LN::BI_RGB, h);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ws.frag(LN::F_RGB + ks, lane), hd[0][ks], acc, 0, 0, 0);
      if (h == 0 && valid) {
        float4 o; o.x = acc[0]; o.y = acc[1]; o.z = acc[2]; o.w = alpha;
        *reinterpret_cast<float4*>(a.out + m * 4) = poison_raw(o, bad);
      }
    }
#undef SINK
#undef MASK_STORE
  }
}

__global__ void __launch_bounds__(512) mlp_small_bwd_kernel(SmallArgs a) {
  constexpr int ST = 1;
  lds_load_stream(a.wb, nullptr);
  const int lane0 = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t ntiles = (a.M + 31) >> 5;
  LdsW ws;
  for (int64_t tile0 = (int64_t)blockIdx.x * 8 + wv; tile0 < ntiles; tile0 += (int64_t)gridDim.x * 8) {
    int lane = lane0;
    asm volatile("" : "+v"(lane));
    const int r = lane & 31, h = lane >> 5;
    const int64_t m = tile0 * 32 + r;
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
    if (m < a.M && h == 0) g = *reinterpret_cast<const float4*>(a.d_raw + m * 4);
    bf16x8 zrgb[ST][1], zal[ST][1];
#pragma unroll
    for (int j = 0; j < 8; ++j) { zrgb[0][0][j] = (__bf16)0.0f; zal[0][0][j] = (__bf16)0.0f; }
    zrgb[0][0][0] = (__bf16)g.x; zrgb[0][0][1] = (__bf16)g.y; zrgb[0][0][2] = (__bf16)g.z;
    zal[0][0][0] = (__bf16)g.w;
    u32x4 mk[3][ST];
#pragma unroll
    for (int l = 0; l < 3; ++l)
      mk[l][0] = *reinterpret_cast<const u32x4*>(frag_ptr(const_cast<void*>(a.acts), tile0, a.astride, LN::A_MASK + l, r, h));
    store_frags<1>(a.dz, tile0, a.zstride, LN::Z_RGB, zrgb[0], r, h);
    store_frags<1>(a.dz, tile0, a.zstride, LN::Z_A, zal[0], r, h);
#define ZSINK(slot0) FragSink<true>{a.dz, tile0, a.zstride, slot0, r, h}
    bf16x8 zd[ST][2], zf[ST][4], z1[ST][4], z0[ST][4];
    layer_bwd<ST, 1, 1, true>(ws, LN::B_RGB, zrgb, zd, mk[2], lane, ZSINK(LN::Z_D));
    layer_bwd<ST, 2, 2, false>(ws, LN::B_DIR, zd, zf, mk[2], lane, ZSINK(LN::Z_F));               // d feature
    {
      bf16x8 cat[ST][5];
#pragma unroll
      for (int k = 0; k < 4; ++k) cat[0][k] = zf[0][k];
      cat[0][4] = zal[0][0];
      layer_bwd<ST, 5, 2, true>(ws, LN::B_FA, cat, z1, mk[1], lane, ZSINK(LN::Z_L1));              // dZ1
    }
    layer_bwd<ST, 4, 2, true>(ws, LN::B_L1, z1, z0, mk[0], lane, ZSINK(LN::Z_L0));                 // dZ0
#undef ZSINK
    if (a.d_x) {                                          // dL/dx = W0^T dZ0, kept in fp32: rows (i&3) + 8 (i>>2) + 4 h
      f32x16 acc;
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
#pragma unroll
      for (int ns = 0; ns < 4; ++ns) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ws.frag(LN::B_L0 + ns, lane), z0[0][ns], acc, 0, 0, 0);
      if (m < a.M) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float4 o; o.x = acc[4 * q]; o.y = acc[4 * q + 1]; o.z = acc[4 * q + 2]; o.w = acc[4 * q + 3];
          *reinterpret_cast<float4*>(a.d_x + m * LN::CPOS + 8 * q + 4 * h) = o;
        }
      }
    }
  }
}

static int g_dw_wgs = 0;       // 0: automatic (see launch_dw)
static int g_dw_bias = -1;     // per-tile fixed cost of a dW job in fragment units (cost model of the static split); -1 = automatic:
                               // 128 for the bf16 kernel (round 2 sweep), 32 for the split-bf16 kernel (round 5: its stage boundary is
                               // paid once per sample tile and narrow jobs use all four SIMDs, so a job's time follows its bytes more
                               // closely: tools/sweep_dw22_bias.py, 3.30-3.34 ms at 16-48 against 3.47 at 128)
static int g_bwd_stage = 0;    // diagnostic: 0 chain + dW, 1 chain only, 2 dW only (on whatever dz holds)
static int g_dw_ring_cap = 8;  // "dw_ring_cap": most stages the 16-wave split-bf16 dW kernel's LDS ring may hold (2 .. 16)
static int g_dw_private = 4;   // "dw_private_tiles": split-bf16 dW jobs of at most this many output tiles run as sixteen wave-private pipelines (0 = off)
static int g_dw16_variant = 1;  // "dw16_variant": bf16 weight gradients: 1 (default) = 256 x 256 jobs on mlp_dww.hip's kernel, tiny-job lists on mlp_s16.hip's, the rest on mlp_dw_kernel; 0 = every job on mlp_dw_kernel; 2 = as 1 without the tiny-job rule; 3 = as 1 with mlp_s16.hip's kernel for every narrow job
static int g_dw_narrow_first = 1;   // "dw_narrow_first": order of the two weight-gradient launches (A/B knob; same gradients either way)
static int g_dw_factor = 1;    // "dw_factor": view model at precision 22: 1 = feature / alpha / dir0 | feature as one shared job + post step (mlp_model.h), 0 = three jobs
static int g_train_fold = 0;   // "train_fold": view model at precision 22 with the factored job list: 1 = the folded split-bf16 training image and kernels (mlp_s16.h), 0 (default) = unfolded
static int g_dw_job_mask = 0;  // diagnostic: nonzero = run only these dW jobs (bit j); view model only
// (g_tile_pad16, "tile_pad16": mlp_model.h, beside the strides it enters)
static int g_mlp_variant = 0;   // 0: auto, 1: ST=1 via L1, 2: ST=2 via L1, 3: LDS ring, 8 waves x 32 samples, 32x32x16 MFMA,
                                // 4: ring, 16x16x32 MFMA, 8 waves x 32 samples (inference only), 5: same, 4 waves x 64 samples
static int g_ring_wgs = 0;       // persistent workgroups of the ring kernels; 0 = one per CU of the current device
static int g_ngp_ray_major = 1;   // A/B knob: fused configs[4] inference query walks (32 rays x 1 depth) tiles (1) or (1 ray x 32 depths) tiles (0)
int g_pass_queue = 1;               // "pass_queue": 1 (default) the persistent ring kernels take their passes from a device-wide counter (mlp_ring.h), 0 = static split
static int g_ring_split = 1;     // training ring kernels: 1 = one 8-wave workgroup per CU (128 KiB ring), 2 = two 4-wave workgroups (64 KiB rings)

// Per-device state.  The CU count (256 on an MI355X in SPX mode; the persistent kernels and the dW split are sized to it instead
// of to a constant) is asked once per device, and the one-time opt-in of a kernel to dynamic LDS above 64 KiB happens inside
// launch<> (launch.h): both belong to the CURRENT device -- a process may move between devices with hipSetDevice, and
// hipFuncSetAttribute applies to the device that is current when it is called.
static int cu_count() {
  constexpr int MAX_DEVICES = 64;
  static int n[MAX_DEVICES] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEVICES) dev = 0;
  if (n[dev] == 0) {
    int v = 0;
    n[dev] = (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) ? v : 256;
  }
  return n[dev];
}
// The weight gradients of the view model at precision 22 run the factored job list (mlp_model.h: VIEW_JOBS_FACTORED) ...
static inline bool dw_factored(const Model& m) { return g_dw_factor && m.can_factor() && !g_dw_job_mask && s16::g_dw_variant != 0; }   // (launch_dw: two launches only)
// ... and only then may its split-bf16 training image be the folded one ("train_fold"): pack, training forward, chain and post step
// all ask here, so the caller sets the option around the calls of one model and a folded image never meets an unfolded kernel.
// Without the factored list the option is ignored.
static inline bool train_folded(const Model& m) { return g_train_fold && dw_factored(m); }
static inline int ring_wgs() { return g_ring_wgs > 0 ? g_ring_wgs : cu_count(); }
// grid of the 8-wave ring kernels: one workgroup per super-tile of 8 tiles, at most one per CU
static inline unsigned ring_grid(int64_t ntiles) { return persistent_grid((ntiles + 7) / 8, ring_wgs()); }

// nerf_set_option / nerf_get_option: one row per key.  rule(v) clamps or normalises the value in place; false = refused with `refusal`.
struct Option { const char* key; int* var; bool (*rule)(int& v); const char* refusal; };
static bool opt_any(int&) { return true; }
static bool opt_flag(int& v) { v = v ? 1 : 0; return true; }
template <int LO, int HI> static bool opt_clamp(int& v) { v = v < LO ? LO : v > HI ? HI : v; return true; }
static const Option OPTIONS[] = {
    {"mlp_variant", &g_mlp_variant, opt_any, nullptr},
    {"ring_split", &g_ring_split, [](int& v) { return v == 1 || v == 2; }, "nerf_set_option: ring_split must be 1 or 2"},
    {"ring_workgroups", &g_ring_wgs, opt_clamp<0, INT_MAX>, nullptr},
    {"tile_pad16", &g_tile_pad16, opt_clamp<0, INT_MAX>, nullptr},
    {"dw_workgroups", &g_dw_wgs, opt_clamp<0, INT_MAX>, nullptr},
    {"dw_unit_bias", &g_dw_bias, opt_clamp<-1, INT_MAX>, nullptr},        // -1 = automatic (a legitimate value: unknown keys are INT_MIN)
    {"bwd_stage", &g_bwd_stage, opt_any, nullptr},
    {"dw_job_mask", &g_dw_job_mask, opt_any, nullptr},
    {"hash_combine_max_res", &g_hash_combine_max_res, opt_clamp<0, INT_MAX>, nullptr},
    {"ngp_ray_major", &g_ngp_ray_major, opt_flag, nullptr},
    {"dw22_variant", &s16::g_dw_variant, opt_flag, nullptr},
    {"dw16_variant", &g_dw16_variant, opt_clamp<0, 3>, nullptr},
    {"dw_private_tiles", &g_dw_private, opt_clamp<0, 4>, nullptr},
    {"dw_ring_cap", &g_dw_ring_cap, opt_clamp<2, 16>, nullptr},
    {"pass_queue", &g_pass_queue, opt_flag, nullptr},
    {"dw_narrow_first", &g_dw_narrow_first, opt_flag, nullptr},
    {"dw_factor", &g_dw_factor, opt_flag, nullptr},
    {"train_fold", &g_train_fold, opt_flag, nullptr},
    {"f22_tiles", &f22::g_tiles, [](int& v) { return v == 0 || v == 2 || v == 3; }, "nerf_set_option: f22_tiles must be 0 (automatic), 2 or 3"},
};

}  // namespace nerf

using namespace nerf;

extern "C" int nerf_set_option(const char* key, int value) {
  NERF_REQUIRE(key, NERF_E_NULL, "nerf_set_option: key is NULL");
  NERF_REQUIRE(strcmp(key, "mlp_precision") != 0, NERF_E_UNSUPPORTED,
               "nerf_set_option: \"mlp_precision\" is gone (ABI 3): set nerf_mlp_arch.precision of the model instead");
  for (const Option& o : OPTIONS) {
    if (strcmp(key, o.key)) continue;
    if (!o.rule(value)) return fail(NERF_E_UNSUPPORTED, "%s", o.refusal);
    *o.var = value;
    return NERF_OK;
  }
  return fail(NERF_E_UNSUPPORTED, "nerf_set_option: unknown key '%s'", key);
}

extern "C" int nerf_get_option(const char* key) {
  if (!key) return NERF_OPTION_UNKNOWN;
  for (const Option& o : OPTIONS)
    if (!strcmp(key, o.key)) return *o.var;
  return NERF_OPTION_UNKNOWN;
}

extern "C" int64_t nerf_mlp_param_count(const nerf_mlp_arch* arch) { return resolve(arch).params; }
extern "C" int64_t nerf_mlp_packed_bytes(const nerf_mlp_arch* arch) { return resolve(arch).packed_bytes; }
extern "C" int64_t nerf_mlp_acts_bytes(const nerf_mlp_arch* arch, int64_t M) { return resolve(arch).acts_bytes(M); }
extern "C" int64_t nerf_mlp_dz_bytes(const nerf_mlp_arch* arch, int64_t M) { return resolve(arch).dz_bytes(M); }

#define NERF_ARCH_MSG ": HIP kernels exist for (8x256, skip 4) with in=63+27 view head, or in=40 / no view head / out_ch<=4, and for (2x64, no skip) with in=32+16 view head"
// declares `m`, the description of `arch`, or returns NERF_E_UNSUPPORTED
#define NERF_RESOLVE(who)        \
  const Model m = resolve(arch); \
  NERF_REQUIRE(m.ok, NERF_E_UNSUPPORTED, who NERF_ARCH_MSG)

extern "C" int nerf_mlp_pack(const nerf_mlp_arch* arch, const float* params, void* packed, void* stream) {
  NERF_RESOLVE("nerf_mlp_pack");
  NERF_REQUIRE(params && packed, NERF_E_NULL, "nerf_mlp_pack: params/packed is NULL");
  auto s = as_stream(stream);
  bf16x8* wf = m.stream<bf16x8>(packed, S_FWD);
  bf16x8* wb = m.stream<bf16x8>(packed, S_BWD);
  float* bias = m.stream<float>(packed, S_BIAS);
  int rc;
  if (m.shape == Shape::Small) {
    rc = launch<pack_streams_kernel<SmallPack, CvtBf16, true>>("nerf_mlp_pack (2x64 model)", dim3(pack_blocks<SmallPack, true>()), dim3(256), 0, s,
                                                               params, wf, wb, bias, 0);
    if (!rc && m.split()) rc = s16x::small_pack(params, m.stream<void>(packed, S_S16), s);
  } else if (m.shape == Shape::Image) {
    rc = launch<pack_streams_kernel<ImgPack, CvtBf16, true>>("nerf_mlp_pack (image model)", dim3(pack_blocks<ImgPack, true>()), dim3(256), 0, s,
                                                             params, wf, wb, bias, m.out_ch);
    if (!rc && m.split()) rc = s16x::img_pack(params, m.out_ch, m.stream<void>(packed, S_S16), s);
    if (!rc && m.prec == Prec::F32) rc = f32::pack(params, m.stream<void>(packed, S_F32), m.out_ch, s);
  } else {
    rc = launch<pack_kernel>("nerf_mlp_pack", dim3(PACK_BLOCKS + PACK16_BLOCKS), dim3(256), 0, s, params, wf, wb, bias,
                             m.stream<bf16x8>(packed, S_FWD16));
    if (!rc && m.prec == Prec::F32) rc = f32::pack(params, m.stream<void>(packed, S_F32), 0, s);
    if (!rc && m.split()) rc = f22::pack(params, m.stream<void>(packed, S_F22), s);
    if (!rc && m.split()) rc = s16::pack(params, m.stream<void>(packed, S_S16), train_folded(m), s);
  }
  return rc;
}

template <int MODE>
static int launch_fwd(const Model& m, const void* packed, const float* x, const float* rays, const float* z, int64_t M, int n,
                      int freq_mode, float* out, void* acts, void* stream) {
  FwdArgs a;
  a.queue = nullptr;
  a.wf = m.stream<bf16x8>(packed, S_FWD);
  a.bias = m.stream<float>(packed, S_BIAS);
  a.x = x; a.rays = rays; a.z = z; a.M = M; a.n = n; a.out = out; a.acts = acts; a.astride = m.astride();
  fill_freqs(a.fr.pos, a.fr.dir, freq_mode);
  const int64_t ntiles = (M + 31) / 32;
  auto s = as_stream(stream);
  // auto: fused query -> LDS ring; the render path (no activations kept) on the 16x16x32 shape, which holds a higher
  // clock: +8 % back to back, +2.5 % inside bench.py's train+render step
  const int variant = (g_mlp_variant == 0) ? (MODE == 1 ? (acts ? 3 : 4) : 1) : g_mlp_variant;
  if ((variant == 4 || variant == 5) && MODE == 1 && !acts) {
    const dim3 g(persistent_grid((M + 255) / 256, ring_wgs()));
    FwdArgs a16 = a;
    a16.queue = passq_slot();
    a16.wf = m.stream<bf16x8>(packed, S_FWD16);
    const char* what = "mlp forward (ring, 16x16x32)";
    if (variant == 4) return launch<mlp_fwd_ring16_kernel<8, 2>, mlp_fwd_ring16_kernel<4, 4>>(what, g, dim3(512), RING16_LDS_BYTES, s, a16);
    return launch<mlp_fwd_ring16_kernel<4, 4>, mlp_fwd_ring16_kernel<8, 2>>(what, g, dim3(256), RING16_LDS_BYTES, s, a16);
  }
  if (variant >= 3 && MODE == 1) {
    a.queue = passq_slot();
    if (acts && g_ring_split == 2) {                      // two 4-wave workgroups per CU, each with its own 64 KiB ring
      return launch<mlp_fwd_ring_kernel<1, true, SPLIT_NW, SPLIT_CHUNK>>(
          "mlp forward (ring, 2 workgroups per CU)", dim3(persistent_grid((ntiles + SPLIT_NW - 1) / SPLIT_NW, 2 * (int64_t)ring_wgs())),
          dim3(64 * SPLIT_NW), SPLIT_LDS_BYTES, s, a);
    }
    return with_bool(acts != nullptr, [&](auto store) {
      constexpr bool ST = decltype(store)::value;
      return launch<mlp_fwd_ring_kernel<1, ST>, mlp_fwd_ring_kernel<1, !ST>>("mlp forward (ring)", dim3(ring_grid(ntiles)), dim3(512),
                                                                              RING_LDS_BYTES, s, a);
    });
  }
  const int st = variant == 2 ? 2 : 1;
  const int64_t blocks = (ntiles + 4 * st - 1) / (4 * st);
  NERF_REQUIRE(blocks < (1ll << 31), NERF_E_SHAPE, "mlp forward: M too large");
  return with_bool(st == 1, [&](auto one) { return with_bool(acts != nullptr, [&](auto store) {
    return launch<mlp_fwd_kernel<decltype(one)::value ? 1 : 2, MODE, decltype(store)::value>>("mlp forward", dim3((unsigned)blocks), dim3(256),
                                                                                                0, s, a);
  }); });
}

// img_args / small_args (kernel arguments of the image / 2 x 64 model from its description): mlp_model.h

// (defined behind nerf_mlp_forward_train: the kernel templates keep the order of first use they always had in the code object)
static int view_forward(const Model& m, const void* packed, const float* x, const float* rays, const float* z, int64_t M, int n,
                        int freq_mode, float* out, void* acts, void* stream);

extern "C" int nerf_mlp_forward_train(const nerf_mlp_arch* arch, const void* packed, const float* x, int64_t M,
                                      float* out, void* acts, void* stream) {
  NERF_RESOLVE("nerf_mlp_forward");
  if (M <= 0) return NERF_OK;
  NERF_REQUIRE(packed && x && out, NERF_E_NULL, "nerf_mlp_forward: NULL pointer");
  auto s = as_stream(stream);
  if (m.shape == Shape::Small) {
    SmallArgs a;
    small_args(a, m, packed);
    a.x = x; a.out = out; a.acts = acts; a.M = M;
    if (m.split()) return s16x::small_forward(a, false, dim3(small_grid(small_tiles(a))), s);      // split bf16: float32-class products (mlp_s16x.hip)
    return with_bool(acts != nullptr, [&](auto store) {
      return launch<mlp_small_fwd_kernel<decltype(store)::value, false>>("mlp forward (2x64 model)", dim3(small_grid((M + 31) / 32)), dim3(512),
                                                                         LN::LDS_BYTES, s, a);
    });
  }
  if (m.shape == Shape::Image) {
    if (m.prec == Prec::F32)                   // float32 operands on the fp32 MFMA (mlp32.hip)
      return f32::forward(m.stream<void>(packed, S_F32), x, nullptr, nullptr, M, 1, 0, out, acts, m.out_ch, s);
    ImgArgs a;
    img_args(a, m, packed);
    a.x = x; a.out = out; a.acts = acts; a.M = M;
    if (m.split()) return s16x::img_forward(a, ring_wgs(), s);
    return with_bool(acts != nullptr, [&](auto store) {
      constexpr bool ST = decltype(store)::value;
      return launch<mlp_img_fwd_ring_kernel<ST>, mlp_img_fwd_ring_kernel<!ST>>("mlp forward (image model)", dim3(ring_grid((M + 31) / 32)),
                                                                               dim3(512), RING_LDS_BYTES, s, a);
    });
  }
  return view_forward(m, packed, x, nullptr, nullptr, M, 1, 0, out, acts, stream);
}

// the view model's forward in its precision; x != nullptr: embedded rows [M,90], else rays + depths (encodings in the kernel)
static int view_forward(const Model& m, const void* packed, const float* x, const float* rays, const float* z, int64_t M, int n,
                        int freq_mode, float* out, void* acts, void* stream) {
  auto s = as_stream(stream);
  if (m.split() && !acts)                      // inference: split fp16 on the 16-bit matrix pipe
    return f22::forward(m.stream<void>(packed, S_F22), x, rays, z, M, n, freq_mode, out, ring_wgs(), s);
  if (m.split())                               // training forward: split bf16, hi + lo fragment blocks kept
    return s16::forward(m.stream<void>(packed, S_S16), m.stream<float>(packed, S_BIAS), x, rays, z, M, n, freq_mode, out, acts,
                        m.astride(), ring_wgs(), train_folded(m), s);
  if (m.prec == Prec::F32) return f32::forward(m.stream<void>(packed, S_F32), x, rays, z, M, n, freq_mode, out, acts, 0, s);
  return x ? launch_fwd<0>(m, packed, x, rays, z, M, n, freq_mode, out, acts, stream)
           : launch_fwd<1>(m, packed, x, rays, z, M, n, freq_mode, out, acts, stream);
}

extern "C" int nerf_mlp_forward(const nerf_mlp_arch* arch, const void* packed, const float* x, int64_t M, float* out,
                                void* stream) {
  return nerf_mlp_forward_train(arch, packed, x, M, out, nullptr, stream);
}

extern "C" int nerf_query_fused(const nerf_mlp_arch* arch, const void* packed, const float* rays, const float* z,
                                int64_t B, int n, int freq_mode, float* raw, void* acts, void* stream) {
  const Model m = resolve(arch);
  NERF_REQUIRE(m.ok && m.shape == Shape::View, NERF_E_UNSUPPORTED, "nerf_query_fused" NERF_ARCH_MSG);
  NERF_REQUIRE(n >= 1, NERF_E_SHAPE, "nerf_query_fused: n must be >= 1");
  if (B <= 0) return NERF_OK;
  NERF_REQUIRE(packed && rays && z && raw, NERF_E_NULL, "nerf_query_fused: NULL pointer");
  NERF_REQUIRE(freq_mode == 0 || freq_mode == 1, NERF_E_UNSUPPORTED, "nerf_query_fused: freq_mode must be 0 or 1");
  NERF_REQUIRE(B * (int64_t)n < (1ll << 31), NERF_E_SHAPE, "nerf_query_fused: B*n must be < 2^31 samples per call");
  return view_forward(m, packed, nullptr, rays, z, B * n, n, freq_mode, raw, acts, stream);
}

// one dW launch + its reduce over a job list.  kind 0: bf16, 16 waves (mlp_dw_kernel); 1: split bf16, 16 waves (s16_dw_kernel);
// 2 / 3: split bf16 / bf16, 256 x 256 jobs only, one wave per SIMD (mlp_dww_kernel).  slot_base: first partial-tile slot of this
// launch (the two launches of one backward pass use disjoint slots).
static int launch_dw_part(const Model& m, DwArgs& d, int nj, int64_t ntiles, const void* acts, void* dz, float* grads,
                          hipStream_t s, int kind, int slot_base, int max_wgs, int aux_slot = -1) {
  static_assert(DW_SPLIT_MAX_JOBS == DW_MAX_JOBS, "dw_split.h sizes its arrays for DwArgs::jobs");
  DwCost cost[DW_MAX_JOBS];
  // The shared job of the factored view model (aux_row0 > 0) multiplies 5 x 8 output tiles for its 25 KiB per half tile, twice the
  // tiles per byte of the other narrow jobs, and the 16-wave kernel runs a stage's reads and MFMAs one after the other: it is costed
  // 12 units above its bytes (training step, blocks of 12 steps, three each: +0 10.13 | +6 10.03 | +12 9.99 | +18 10.03 | +24 10.07 ms).
  constexpr int SHARED_JOB_EXTRA_UNITS = 12;
  for (int j = 0; j < nj; ++j) cost[j] = DwCost{d.jobs[j].nf, d.jobs[j].kf + (d.jobs[j].aux_row0 > 0 ? SHARED_JOB_EXTRA_UNITS : 0)};
  // the cost model and the largest-remainder split: dw_split.h.  "dw_workgroups" overrides the total.
  int target_wgs = g_dw_wgs > 0 ? g_dw_wgs : cu_count();
  if (target_wgs > max_wgs) target_wgs = max_wgs;               // one partial-tile slot per workgroup
  const int nw = dw_split(cost, nj, g_dw_bias >= 0 ? g_dw_bias : m.split() ? 2 : 128, target_wgs, (ntiles + 3) / 4, d.splits);
  NERF_REQUIRE(slot_base + nw <= DW_MAX_WGS, NERF_E_SHAPE, "nerf_mlp_backward: dw_workgroups must be <= %d", DW_MAX_WGS);
  bool all_tiny = true;
  for (int j = 0; j < nj; ++j) all_tiny = all_tiny && ((d.jobs[j].nf + 1) / 2) * ((d.jobs[j].kf + 1) / 2) <= 4;
  d.ntiles = (int)ntiles; d.astride = m.astride(); d.zstride = m.zstride();
  d.acts = acts; d.dz = dz; d.grads = grads;
  d.a_lo = m.info->a_lo; d.z_lo = m.info->z_lo; d.ring_cap = g_dw_ring_cap; d.private_max_tiles = g_dw_private;
  // the partial-tile slots live behind the dZ fragment blocks in the caller's dz workspace (nerf_mlp_dz_bytes counts them)
  d.partial = m.dw_partial(dz, ntiles) + (size_t)slot_base * DW_SLOT_FLOATS;
  d.aux = aux_slot >= 0 ? m.dw_partial(dz, ntiles) + (size_t)aux_slot * DW_SLOT_FLOATS : nullptr;
  int rc;
  if (kind >= 2) {             // 16 x 16-fragment jobs, one wave per SIMD (mlp_dww.hip); same slots and reduce
    rc = launch_dw_wide_kernel(d, nw, kind == 2, s);
  } else if (kind == 1) {      // hi + lo fragment blocks, three MFMAs per product (mlp_s16.hip); same jobs, slots and reduce
    rc = s16::launch_dw_kernel(d, nw, true, s);
  } else if (g_dw16_variant == 3 || (g_dw16_variant == 1 && all_tiny)) {
    // the 16-wave kernel of mlp_s16.hip over the bf16 stores: for job lists of tiny jobs only (the 2 x 64 model: sixteen wave-private
    // pipelines, configs[4] bf16 training 3.10 -> 3.21 M rays/s).  For the view model's narrow jobs it measures like round 2's
    // mlp_dw_kernel below (4.45 against 4.43 ms per training step), which keeps them ("dw16_variant" 3 forces this kernel).
    rc = s16::launch_dw_kernel(d, nw, false, s);
  } else {
    rc = launch<mlp_dw_kernel>("mlp dW", dim3(nw), dim3(64 * DW_WAVES), DW_LDS_BYTES, s, d);
  }
  if (rc) return rc;
  return launch<mlp_dw_reduce_kernel>("mlp dW reduce", dim3(257, nj), dim3(256), 0, s, d);        // 256 x 256 weights + 256 biases: one element per thread
}

// split the (dZ, H) jobs over workgroups and launch the dW kernel(s); grads[0..m.params) is overwritten.
// factored: d.jobs is the view model's factored list (mlp_model.h).  Its shared job is a narrow one; the reduce of the narrow launch
// leaves G and db_D in the FIRST partial-tile slot of the wide launch's half, which is idle then in either order of the two launches
// (not yet written, or already reduced: the stream serialises them), and the post step runs directly behind that reduce, in front of
// whatever the wide launch does next.  No byte of workspace is added.  The one-launch form ("dw22_variant" 0) may use all slots, so
// the caller keeps the legacy table there.
static int launch_dw(const Model& m, const void* packed, DwArgs& d, int nj, int64_t ntiles, const void* acts, void* dz, float* grads,
                     hipStream_t s, bool factored) {
  if (g_dw_job_mask) {          // diagnostic subset of jobs: the parameters of the jobs left out read as zero
    hipError_t e = hipMemsetAsync(grads, 0, sizeof(float) * m.params, s);
    if (e != hipSuccess) return fail(NERF_E_HIP, "nerf_mlp_backward: memset: %s", hipGetErrorString(e));
  }
  // "dw22_variant" / "dw16_variant" 1 (default): the 256 x 256 jobs on the one-wave-per-SIMD kernel, the others on the 16-wave kernel;
  // two launches, each with its own static split over all CUs and its own half of the partial-tile slots.  0: one 16-wave launch.
  const bool split_bf16 = m.split();
  if ((split_bf16 ? s16::g_dw_variant : g_dw16_variant) == 0)
    return launch_dw_part(m, d, nj, ntiles, acts, dz, grads, s, split_bf16 ? 1 : 0, 0, DW_MAX_WGS);
  DwArgs wide = d, rest = d;
  int nwide = 0, nrest = 0;
  for (int j = 0; j < nj; ++j) {
    if (d.jobs[j].nf == 16 && d.jobs[j].kf == 16) wide.jobs[nwide++] = d.jobs[j];
    else rest.jobs[nrest++] = d.jobs[j];
  }
  const int half = DW_MAX_WGS / 2;
  for (int turn = 0; turn < 2; ++turn) {        // "dw_narrow_first" 1: the load-bound narrow jobs before the MFMA-bound 256 x 256 jobs
    const bool do_wide = (turn == 0) != (g_dw_narrow_first != 0);
    if (do_wide && nwide) {
      const int rc = launch_dw_part(m, wide, nwide, ntiles, acts, dz, grads, s, split_bf16 ? 2 : 3, half, half);
      if (rc) return rc;
    }
    if (!do_wide && nrest) {
      int rc = launch_dw_part(m, rest, nrest, ntiles, acts, dz, grads, s, split_bf16 ? 1 : 0, 0, half, factored ? half : -1);
      if (!rc && factored)
        rc = launch_dw_factor_post(m.stream<void>(packed, S_S16), m.stream<float>(packed, S_BIAS), rest.aux, grads, train_folded(m), s);
      if (rc) return rc;
    }
  }
  return NERF_OK;
}

// the dZ chain of the view model (bf16 or split bf16)
static int view_backward_chain(const Model& m, const void* packed, const void* acts, const float* d_raw, int64_t M, void* dz,
                               hipStream_t s) {
  const int64_t ntiles = (M + 31) / 32;
  if (m.split()) {
    if (g_bwd_stage != 2) {
      const int rcs = s16::backward_chain(m.stream<void>(packed, S_S16), acts, d_raw, M, dz, m.astride(), m.zstride(), ring_wgs(), train_folded(m), s);
      if (rcs) return rcs;
    }
    return check_launch("mlp backward chain");
  }
  BwdArgs b;
  b.queue = nullptr;
  b.wb = m.stream<bf16x8>(packed, S_BWD);
  b.acts = acts; b.d_raw = d_raw; b.M = M; b.dz = dz; b.astride = m.astride(); b.zstride = m.zstride();
  const int variant = g_mlp_variant == 0 ? 3 : g_mlp_variant;
  const char* what = "mlp backward chain";
  if (variant >= 3) {
    b.queue = passq_slot();
    if (g_bwd_stage == 2) return check_launch(what);
    if (g_ring_split == 2)
      return launch<mlp_bwd_ring_kernel<SPLIT_NW, SPLIT_CHUNK>>(
          what, dim3(persistent_grid((ntiles + SPLIT_NW - 1) / SPLIT_NW, 2 * (int64_t)ring_wgs())), dim3(64 * SPLIT_NW), SPLIT_LDS_BYTES, s, b);
    return launch<mlp_bwd_ring_kernel<>>(what, dim3(ring_grid(ntiles)), dim3(512), RING_LDS_BYTES, s, b);
  }
  const int st = variant == 2 ? 2 : 1;
  const int64_t blocks = (ntiles + 4 * st - 1) / (4 * st);
  return with_bool(st == 1, [&](auto one) {
    return launch<mlp_bwd_kernel<decltype(one)::value ? 1 : 2>>(what, dim3((unsigned)blocks), dim3(256), 0, s, b);
  });
}

static int mlp_backward_impl(const nerf_mlp_arch* arch, const void* packed, const void* acts, const float* d_raw,
                             int64_t M, void* dz, float* grads, float* d_x, void* stream) {
  NERF_RESOLVE("nerf_mlp_backward");
  NERF_REQUIRE(!d_x || m.shape == Shape::Small, NERF_E_UNSUPPORTED,
               "nerf_mlp_backward_inputs: input gradients exist for the (2x64) model only (the 8x256 models take fixed encodings)");
  NERF_REQUIRE(packed && acts && d_raw && dz && grads, NERF_E_NULL, "nerf_mlp_backward: NULL pointer");
  NERF_REQUIRE(M > 0, NERF_E_SHAPE, "nerf_mlp_backward: M must be > 0");
  auto s = as_stream(stream);
  const int64_t ntiles = (M + 31) / 32;
  if (m.prec == Prec::F32)                     // mlp32.hip: chain and dW in its own store format
    return f32::backward(m.stream<void>(packed, S_F32), acts, d_raw, M, dz, grads, m.shape == Shape::Image ? m.out_ch : 0, s);
  // ---- 1. dZ chain
  int rc;
  if (m.shape == Shape::Small) {
    SmallArgs a;
    small_args(a, m, packed);
    a.d_raw = d_raw; a.acts = const_cast<void*>(acts); a.dz = dz; a.M = M; a.d_x = d_x;
    if (m.split()) rc = s16x::small_backward_chain(a, s);
    else rc = launch<mlp_small_bwd_kernel>("mlp backward chain (2x64 model)", dim3(small_grid(ntiles)), dim3(512), LN::LDS_BYTES, s, a);
  } else if (m.shape == Shape::Image) {
    ImgArgs a;
    img_args(a, m, packed);
    a.d_out = d_raw; a.acts = const_cast<void*>(acts); a.dz = dz; a.M = M;
    if (m.split()) rc = s16x::img_backward_chain(a, ring_wgs(), s);
    else rc = launch<mlp_img_bwd_ring_kernel>("mlp backward chain (image model)", dim3(ring_grid(ntiles)), dim3(512), RING_LDS_BYTES, s, a);
  } else {
    rc = view_backward_chain(m, packed, acts, d_raw, M, dz, s);
    if (!rc && g_bwd_stage == 1) return NERF_OK;
  }
  if (rc) return rc;
  // ---- 2. dW / db
  DwArgs d;
  const int mask = m.shape == Shape::View ? g_dw_job_mask : 0;
  const bool factored = dw_factored(m);
  const int nj = m.dw_jobs(d.jobs, mask, factored);
  return launch_dw(m, packed, d, nj, ntiles, acts, dz, grads, s, factored);
}

// lw_host: the level weights of nerf_ngp_query_fused_lw; NULL = the kernels without them
static int ngp_query_fused_impl(const nerf_mlp_arch* arch, const void* packed, const float* rays, const float* z,
                                int64_t B, int n, const float* tables, const void* tables_half, int L, int log2_T, int F,
                                const int* resolutions_host, const float* lw_host, int sh_degree, float pos_scale,
                                float pos_offset, float* raw, void* acts, void* stream) {
  const Model m = resolve(arch);
  NERF_REQUIRE(m.ok && m.shape == Shape::Small, NERF_E_UNSUPPORTED, "nerf_ngp_query_fused: needs the (2x64, in 32+16) model");
  NERF_REQUIRE(L == 16 && F == 2 && sh_degree == 3, NERF_E_UNSUPPORTED,
               "nerf_ngp_query_fused: fused rows exist for 16 levels x 2 features + SH degree 3 (use nerf_ngp_encode + nerf_mlp_forward otherwise)");
  NERF_REQUIRE(log2_T >= 1 && log2_T <= 30, NERF_E_SHAPE, "nerf_ngp_query_fused: need 1<=log2_T<=30");
  if (B <= 0 || n <= 0) return NERF_OK;
  NERF_REQUIRE(packed && rays && z && tables && resolutions_host && raw, NERF_E_NULL, "nerf_ngp_query_fused: NULL pointer");
  const int64_t M = B * n;
  NERF_REQUIRE(M < (1ll << 31), NERF_E_SHAPE, "nerf_ngp_query_fused: B*n must be < 2^31");
  LevelTab lt;
  if (lw_host)
    NERF_REQUIRE(level_tab_fill(lt, lw_host, L), NERF_E_SHAPE, "nerf_ngp_query_fused_lw: level weights must be finite and in [0, 1]");
  SmallArgs a;
  small_args(a, m, packed);
  a.out = raw; a.acts = acts; a.M = M; a.rays = rays; a.z = z; a.n = n; a.tables = tables; a.T = 1u << log2_T;
  a.pos_scale = pos_scale; a.pos_offset = pos_offset;
  for (int l = 0; l < L; ++l) a.rt.res[l] = (float)resolutions_host[l];
  if (lw_host) a.lw = lt;
  a.B = B;
  a.ray_major = small_ray_major(acts != nullptr, g_ngp_ray_major, B);
  const dim3 g(small_grid(small_tiles(a)));
  // precision 22 is the reference's tolerance: float32 gathers from the master tables (the fp16 shadow is a reduced-precision
  // image: not read in this mode), float32 interpolation, split-bf16 MLP (mlp_s16x.hip)
  if (m.split()) return s16x::small_forward(a, lw_host != nullptr, g, as_stream(stream));
  a.tables_h = static_cast<const uint32_t*>(tables_half);
  return with_bool(acts != nullptr, [&](auto store) { return with_bool(lw_host != nullptr, [&](auto lw) {
    return launch<mlp_small_fwd_kernel<decltype(store)::value, true, decltype(lw)::value>>(
        lw_host ? "nerf_ngp_query_fused_lw" : "nerf_ngp_query_fused", g, dim3(512), LN::LDS_BYTES, as_stream(stream), a);
  }); });
}

extern "C" int nerf_ngp_query_fused_h(const nerf_mlp_arch* arch, const void* packed, const float* rays, const float* z,
                                      int64_t B, int n, const float* tables, const void* tables_half, int L, int log2_T, int F,
                                      const int* resolutions_host, int sh_degree, float pos_scale, float pos_offset,
                                      float* raw, void* acts, void* stream) {
  return ngp_query_fused_impl(arch, packed, rays, z, B, n, tables, tables_half, L, log2_T, F, resolutions_host, nullptr, sh_degree,
                              pos_scale, pos_offset, raw, acts, stream);
}

extern "C" int nerf_ngp_query_fused_lw(const nerf_mlp_arch* arch, const void* packed, const float* rays, const float* z,
                                       int64_t B, int n, const float* tables, const void* tables_half, int L, int log2_T, int F,
                                       const int* resolutions_host, const float* level_weights_host, int sh_degree,
                                       float pos_scale, float pos_offset, float* raw, void* acts, void* stream) {
  return ngp_query_fused_impl(arch, packed, rays, z, B, n, tables, tables_half, L, log2_T, F, resolutions_host, level_weights_host,
                              sh_degree, pos_scale, pos_offset, raw, acts, stream);
}

extern "C" int nerf_ngp_query_fused(const nerf_mlp_arch* arch, const void* packed, const float* rays, const float* z,
                                    int64_t B, int n, const float* tables, int L, int log2_T, int F,
                                    const int* resolutions_host, int sh_degree, float pos_scale, float pos_offset,
                                    float* raw, void* acts, void* stream) {
  return nerf_ngp_query_fused_h(arch, packed, rays, z, B, n, tables, nullptr, L, log2_T, F, resolutions_host, sh_degree, pos_scale,
                                pos_offset, raw, acts, stream);
}

extern "C" int nerf_mlp_backward(const nerf_mlp_arch* arch, const void* packed, const void* acts, const float* d_raw,
                                 int64_t M, void* dz, float* grads, void* stream) {
  return mlp_backward_impl(arch, packed, acts, d_raw, M, dz, grads, nullptr, stream);
}

extern "C" int nerf_mlp_backward_inputs(const nerf_mlp_arch* arch, const void* packed, const void* acts,
                                        const float* d_raw, int64_t M, void* dz, float* grads, float* d_x,
                                        void* stream) {
  NERF_REQUIRE(d_x, NERF_E_NULL, "nerf_mlp_backward_inputs: d_x is NULL");
  return mlp_backward_impl(arch, packed, acts, d_raw, M, dz, grads, d_x, stream);
}

// ---- test hook: one layer of the training stores (fragment blocks) as row-major fp32 ----------------------------
namespace nerf {
__global__ void __launch_bounds__(256) decode_frags_kernel(const void* base, int64_t stride16, int slot0, int nfrag,
                                                           int64_t M, float* __restrict__ out, int lo_off) {
  const int64_t total = M * nfrag * 2;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int h = (int)(t & 1), ks = (int)((t >> 1) % nfrag);
    const int64_t m = t / (2 * nfrag);
    const bf16x8 v = *frag_ptr(const_cast<void*>(base), m >> 5, stride16, slot0 + ks, (int)(m & 31), h);
#pragma unroll
    for (int j = 0; j < 8; ++j) out[m * (16 * nfrag) + kperm(ks, h, j)] = (float)v[j];
    if (lo_off > 0) {           // split-bf16 stores: value = hi block + lo block
      const bf16x8 w = *frag_ptr(const_cast<void*>(base), m >> 5, stride16, slot0 + lo_off + ks, (int)(m & 31), h);
#pragma unroll
      for (int j = 0; j < 8; ++j) out[m * (16 * nfrag) + kperm(ks, h, j)] += (float)w[j];
    }
  }
}
}  // namespace nerf

extern "C" int nerf_mlp_debug_width(const nerf_mlp_arch* arch, int kind, int layer) {
  const Model m = resolve(arch);
  if (!m.ok) return -1;
  if (m.prec == Prec::F32) return f32::debug_width(kind, layer);
  const DebugSlot ds = m.debug_slot(kind, layer);
  return ds.nfrag ? 16 * ds.nfrag : -1;
}

extern "C" int nerf_mlp_debug_read(const nerf_mlp_arch* arch, const void* store, int kind, int layer, int64_t M,
                                   float* out, void* stream) {
  NERF_RESOLVE("nerf_mlp_debug_read");
  if (m.prec == Prec::F32) {
    NERF_REQUIRE(store && out, NERF_E_NULL, "nerf_mlp_debug_read: NULL pointer");
    return M <= 0 ? NERF_OK : f32::debug_read(store, kind, layer, M, out, as_stream(stream));
  }
  const DebugSlot ds = m.debug_slot(kind, layer);
  NERF_REQUIRE(ds.nfrag, NERF_E_SHAPE, "nerf_mlp_debug_read: no such (kind, layer) in this architecture's stores");
  NERF_REQUIRE(store && out, NERF_E_NULL, "nerf_mlp_debug_read: NULL pointer");
  if (M <= 0) return NERF_OK;
  const int lo_off = !m.split() ? 0 : kind == 0 ? m.info->a_lo : m.info->z_lo;       // split-bf16 stores: value = hi block + lo block
  return launch<decode_frags_kernel>("nerf_mlp_debug_read", dim3(grid_for(M * ds.nfrag * 2, 256)), dim3(256), 0, as_stream(stream), store,
                                     kind == 0 ? m.astride() : m.zstride(), ds.slot, ds.nfrag, M, out, lo_off);
}

NERF_STAMP2_EXPORT(nerf_debug_stamps2_ring16)
#ifdef NERF_CLOCK_STAMP
extern "C" int nerf_debug_stamps(unsigned long long* host_out, int nwg) {
  if (nwg > 4096) nwg = 4096;
  return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(nerf::g_stamps), (size_t)nwg * 32) == hipSuccess ? 0 : -4;
}
#endif
