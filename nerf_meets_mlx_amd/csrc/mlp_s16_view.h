// Split-bf16 training forward and dZ chain of the 8 x 256 view model: the device code shared by the two translation units that
// instantiate it -- mlp_s16.hip (the unfolded form, FOLD = false) and mlp_s16f.hip (the folded form, FOLD = true: mlp_s16.h).  One
// unit per form, so that each object's ISA is scanned on its own (Makefile: check_m0.py --no-scratch) and the unfolded unit holds the
// kernels it always held.  Arithmetic and scheme: mlp_s16.hip.
#pragma once
#include <type_traits>
#include "mlp_s16_dev.h"
#include "mlp_s16.h"

// 1: the training forward re-reads its own stored encodings before pos5 / dir0 (48 registers less to carry through pos1..4; a
// compiler-counted global load, i.e. a vmcnt(0) that drains the ring's DMAs and the pending stores); 0: keeps them (the 512-register
// file of a one-wave-per-SIMD kernel has the room: they live in AGPRs)
#ifndef NERF_S16_RELOAD_PE
#define NERF_S16_RELOAD_PE 0
#endif

namespace nerf {
namespace s16 {

constexpr int F_CHUNKS = F_FRAGS / RING_CHUNK;          // 74
constexpr int B_CHUNKS = B_PADDED / RING_CHUNK;         // 69
static_assert(F_CHUNKS * RING_CHUNK == F_FRAGS && B_CHUNKS * RING_CHUNK == B_PADDED, "whole ring chunks");
static_assert(F_FRAGS == 2 * L::F_TOTAL && B_FRAGS == 2 * L::B_TOTAL, "pair streams");
static_assert(A_LO == L::A_MASK && A_MASK == 2 * L::A_MASK && A_SLOTS == A_MASK + 9, "activation slots");
static_assert(Z_LO == L::Z_SLOTS && Z_SLOTS == 2 * L::Z_SLOTS, "dZ slots");
constexpr int NW = 4;                                    // waves per workgroup of the forward / chain kernels

typedef RingW<F_CHUNKS, F_FRAGS, 4, NW, RING_CHUNK, RING_STAGES, true> FwdRing;      // DMA runs of four (mlp_ring.h)
typedef RingW<B_CHUNKS, B_FRAGS, 4, NW, RING_CHUNK, RING_STAGES, true> BwdRing;
// the folded form (mlp_index.h, namespace LF): 2 x 1056 and 2 x 972 fragments
constexpr int FF_FRAGS = 2 * LF::F_TOTAL, FB_FRAGS = 2 * LF::B_TOTAL, FB_PADDED = 2 * LF::B_PADDED;
constexpr int FF_CHUNKS = FF_FRAGS / RING_CHUNK;         // 66
constexpr int FB_CHUNKS = FB_PADDED / RING_CHUNK;        // 61
typedef RingW<FF_CHUNKS, FF_FRAGS, 4, NW, RING_CHUNK, RING_STAGES, true> FwdRingFold;
typedef RingW<FB_CHUNKS, FB_FRAGS, 4, NW, RING_CHUNK, RING_STAGES, true> BwdRingFold;
// A ring wraps modulo its chunk count at the end of a pass: the count must be the chunks one pass CONSUMES, ceil(fragments / chunk)
// -- one more and a workgroup's second pass runs on shifted weights (the image model's chain once did).
constexpr int ring_chunks(int frags) { return (frags + RING_CHUNK - 1) / RING_CHUNK; }
static_assert(F_CHUNKS == ring_chunks(F_FRAGS) && B_CHUNKS == ring_chunks(B_FRAGS), "ring chunk counts of the unfolded streams");
static_assert(FF_CHUNKS == ring_chunks(FF_FRAGS) && FB_CHUNKS == ring_chunks(FB_FRAGS), "ring chunk counts of the folded streams");
static_assert(FF_CHUNKS * RING_CHUNK == FF_FRAGS && FB_CHUNKS * RING_CHUNK == FB_PADDED && FB_PADDED >= FB_FRAGS, "whole ring chunks (folded)");
static_assert(FF_FRAGS % 4 == 0 && FB_FRAGS % 4 == 0, "a pass is whole fragment groups");
static_assert(FF_FRAGS == F_FRAGS - 256 && FB_FRAGS == B_FRAGS - 256, "the fold removes 128 pairs from each stream");
static_assert((int64_t)LF::C_END * 4 == PACKED_BYTES && (int64_t)LF::C_WFT * 4 == (int64_t)FF_FRAGS * 1024 &&
              (int64_t)LF::C_WD1 * 4 == (int64_t)(F_FRAGS + FB_PADDED) * 1024, "the fp32 copies start where the folded streams end");


// positional encodings (within 6e-7 of the float64 sine before the split), straight into (hi, lo) B fragments: mlp_input.h (here: SinCodyWaite, SplitBf16)

// All 12 layers for the wave's 32 samples (sample tile `tile0`).  Waves past the end compute on clamped inputs, store into
// the padding tiles of the workspace and write no output, so every wave runs the same instruction stream (the ring needs it).
// MODE 0: embedded rows;  MODE 1: rays + z with fused positional encodings
// FOLD: the folded stream (mlp_s16.h) -- no feature layer, dir0' reads h7
template <int MODE, bool FOLD, class WS>
__device__ __forceinline__ void fwd_tiles(const FwdArgs& a, WS& ws, int64_t tile0, int64_t ntiles, int lane, PassQueue& pq) {
  const int r = lane & 31, h = lane >> 5;
  bf16x8 peh[4], pel[4], dph[2], dpl[2];
  pq.ask(ws.wv, lane);                    // dynamic pass queue (mlp_ring.h): before this pass's input loads
  {
    const int64_t tile = tile0 < ntiles ? tile0 : ntiles - 1;
    const int64_t m = clamp_sample(tile * 32 + r, a.M);
    if (MODE == 0) {
      const float* row = a.x + m * 90;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) row_pairs<SplitBf16>(row, ks, h, 63, peh[ks], pel[ks]);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) row_pairs<SplitBf16>(row + 63, ks, h, 27, dph[ks], dpl[ks]);
    } else {
      const Sample sm = load_sample(a.rays, a.z, m, a.n);
      encode_pairs<SinCodyWaite, SplitBf16, 0, 63, 10>(sm.p, a.fr.pos, h, peh[0], pel[0]); encode_pairs<SinCodyWaite, SplitBf16, 1, 63, 10>(sm.p, a.fr.pos, h, peh[1], pel[1]);
      encode_pairs<SinCodyWaite, SplitBf16, 2, 63, 10>(sm.p, a.fr.pos, h, peh[2], pel[2]); encode_pairs<SinCodyWaite, SplitBf16, 3, 63, 10>(sm.p, a.fr.pos, h, peh[3], pel[3]);
      encode_pairs<SinCodyWaite, SplitBf16, 0, 27, 4>(sm.d, a.fr.dir, h, dph[0], dpl[0]); encode_pairs<SinCodyWaite, SplitBf16, 1, 27, 4>(sm.d, a.fr.dir, h, dph[1], dpl[1]);
    }
  }
  pq.publish(ws.wv);
  store_frags<4>(a.acts, tile0, a.astride, L::A_PE, peh, r, h); store_frags<4>(a.acts, tile0, a.astride, A_LO + L::A_PE, pel, r, h);
  store_frags<2>(a.acts, tile0, a.astride, L::A_DPE, dph, r, h); store_frags<2>(a.acts, tile0, a.astride, A_LO + L::A_DPE, dpl, r, h);

  bf16x8 hah[16], hal[16], hbh[16], hbl[16];
  u32x4 mk;
#define SINK(slot0) PairSink{a.acts, tile0, a.astride, slot0, A_LO, r, h}
#define MASK_BEGIN() mk = u32x4{0u, 0u, 0u, 0u}
#define MASK_STORE(layer) *reinterpret_cast<u32x4*>(frag_ptr(a.acts, tile0, a.astride, A_MASK + (layer), r, h)) = mk
  MASK_BEGIN();
  layer_fwd<4, 8, true, true>(ws, L::F_L0, 0, peh, pel, hah, hal, mk, lane, SINK(L::A_H0));
  MASK_STORE(0);
  MASK_BEGIN();
  layer_fwd<16, 8, true, true>(ws, L::F_L1 + 0 * 128, 256, hah, hal, hbh, hbl, mk, lane, SINK(L::A_H0 + 16));
  MASK_STORE(1);
  MASK_BEGIN();
  layer_fwd<16, 8, true, true>(ws, L::F_L1 + 1 * 128, 512, hbh, hbl, hah, hal, mk, lane, SINK(L::A_H0 + 32));
  MASK_STORE(2);
  MASK_BEGIN();
  layer_fwd<16, 8, true, true>(ws, L::F_L1 + 2 * 128, 768, hah, hal, hbh, hbl, mk, lane, SINK(L::A_H0 + 48));
  MASK_STORE(3);
  MASK_BEGIN();
  layer_fwd<16, 8, true, true>(ws, L::F_L1 + 3 * 128, 1024, hbh, hbl, hah, hal, mk, lane, SINK(L::A_H0 + 64));
  MASK_STORE(4);
  {                                                           // pos5 on concat[input_pos, h]  (models/NeRF.py:224-225)
    bf16x8 cth[20], ctl[20];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#if NERF_S16_RELOAD_PE                                        // register relief: the encoding was just stored
      cth[k] = *frag_ptr(a.acts, tile0, a.astride, L::A_PE + k, r, h);
      ctl[k] = *frag_ptr(a.acts, tile0, a.astride, A_LO + L::A_PE + k, r, h);
#else
      cth[k] = peh[k]; ctl[k] = pel[k];
#endif
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) { cth[4 + k] = hah[k]; ctl[4 + k] = hal[k]; }
    MASK_BEGIN();
    layer_fwd<20, 8, true, true>(ws, L::F_L5, 1280, cth, ctl, hbh, hbl, mk, lane, SINK(L::A_H0 + 80));
    MASK_STORE(5);
  }
  MASK_BEGIN();
  layer_fwd<16, 8, true, true>(ws, L::F_L6, 1536, hbh, hbl, hah, hal, mk, lane, SINK(L::A_H0 + 96));
  MASK_STORE(6);
  MASK_BEGIN();
  layer_fwd<16, 8, true, true>(ws, L::F_L7, 1792, hah, hal, hbh, hbl, mk, lane, SINK(L::A_H0 + 112));
  MASK_STORE(7);
  // feature (no activation) and alpha (row 0 of a ninth tile)   models/NeRF.py:229-231
  if constexpr (!FOLD) layer_fwd<16, 8, false, false>(ws, L::F_FA, L::BI_FEAT, hbh, hbl, hah, hal, mk, lane, SINK(L::A_FEAT));
  const float alpha = head<16>(ws, FOLD ? LF::F_A : L::F_FA + 128, L::BI_ALPHA, hbh, hbl, lane)[0];
  // view branch: relu(Linear([feature, input_dir]))  then rgb   models/NeRF.py:232-238
  bf16x8 hdh[8], hdl[8];
  {
    bf16x8 cth[18], ctl[18];
#pragma unroll
    for (int k = 0; k < 16; ++k) { cth[k] = FOLD ? hbh[k] : hah[k]; ctl[k] = FOLD ? hbl[k] : hal[k]; }     // FOLD: h7 through W'
#pragma unroll
    for (int k = 0; k < 2; ++k) {
#if NERF_S16_RELOAD_PE
      cth[16 + k] = *frag_ptr(a.acts, tile0, a.astride, L::A_DPE + k, r, h);
      ctl[16 + k] = *frag_ptr(a.acts, tile0, a.astride, A_LO + L::A_DPE + k, r, h);
#else
      cth[16 + k] = dph[k]; ctl[16 + k] = dpl[k];
#endif
    }
    MASK_BEGIN();
    layer_fwd<18, 4, true, true>(ws, FOLD ? LF::F_DIR : L::F_DIR, L::BI_DIR, cth, ctl, hdh, hdl, mk, lane, SINK(L::A_HD));
    MASK_STORE(8);
  }
  const f32x16 rgb = head<8>(ws, FOLD ? LF::F_RGB : L::F_RGB, L::BI_RGB, hdh, hdl, lane);
  const int64_t m = tile0 * 32 + r;
  if (h == 0 && tile0 < ntiles && m < a.M) {
    float4 o; o.x = rgb[0]; o.y = rgb[1]; o.z = rgb[2]; o.w = alpha;     // [rgb, alpha] raw (:239)
    *reinterpret_cast<float4*>(a.out + m * 4) = o;
  }
#undef SINK
#undef MASK_BEGIN
#undef MASK_STORE
}

template <int MODE, bool FOLD>
__global__ void __launch_bounds__(64 * NW) s16_fwd_kernel(FwdArgs a) {
  typedef std::conditional_t<FOLD, FwdRingFold, FwdRing> Ring;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t ntiles = (a.M + 31) >> 5, nsuper = (ntiles + NW - 1) / NW;
  Ring ws;
  ws.wsrc = reinterpret_cast<const char*>(a.wf);
  ws.lane16 = 16 * lane;
  ws.lds0 = __builtin_amdgcn_readfirstlane(lds_addr_of(ring_smem));
  ws.wv = wv;
  ws.start(lane);
  if constexpr (FOLD) {                   // dir0's bias slots hold b' (the image's fp32 copy); the feature slots are not read
    const float* bp = reinterpret_cast<const float*>(a.wf) + LF::C_BP;
    for (int i = threadIdx.x; i < L::BI_TOTAL; i += blockDim.x) {
      const bool dir = i >= L::BI_DIR && i < L::BI_DIR + 128;
      *reinterpret_cast<float*>(ring_smem + Ring::BIAS_OFF + 4 * i) = dir ? bp[i - L::BI_DIR] : a.bias[i];
    }
  } else ring_load_bias(a.bias, L::BI_TOTAL, Ring::BIAS_OFF);
  __syncthreads();
  PassQueue pq;                           // dynamic pass queue (mlp_ring.h); a.queue == nullptr: static split
  pq.init(a.queue, ws.lds0 + Ring::BIAS_OFF);
  for (int64_t sp = blockIdx.x; sp < nsuper;) {
    int ln = lane;
    asm volatile("" : "+v"(ln));          // lane-derived values are recomputed per pass, not hoisted and spilled
    ws.new_pass();
    fwd_tiles<MODE, FOLD>(a, ws, sp * NW + wv, ntiles, ln, pq);
    sp = pq.next(sp);
  }
  ws.drain();                             // the ring always runs 3 chunks ahead
  pq.leave();
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

// FOLD: the folded transposed stream -- [dZ_D | d alpha] -> dZ7 through [W'^T | W_A^T] in one step, no dZ_F
template <bool FOLD, class WS>
__device__ __forceinline__ void bwd_tiles(const BwdArgs& a, WS& ws, int64_t tile0, int64_t ntiles, int lane, PassQueue& pq) {
  const int r = lane & 31, h = lane >> 5;
  const bool live = tile0 < ntiles;
  pq.ask(ws.wv, lane);                    // dynamic pass queue (mlp_ring.h): before this pass's input loads
  const int64_t tile = live ? tile0 : ntiles - 1;
  bf16x8 zrh[1], zrl[1], zah[1], zal[1];
  {
    const int64_t m = tile * 32 + r;
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live && m < a.M && h == 0) g = *reinterpret_cast<const float4*>(a.d_raw + m * 4);
    float vr[8] = {g.x, g.y, g.z, 0.f, 0.f, 0.f, 0.f, 0.f}, va[8] = {g.w, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    split_slots<8>(vr, zrh, zrl);                         // rows 0..2 (h == 0)
    split_slots<8>(va, zah, zal);                         // row 0
  }
  pq.publish(ws.wv);
  // every ReLU mask of the pass is fetched here, so the chain itself issues no loads the compiler must wait for
  u32x4 mk[9];
#pragma unroll
  for (int l = 0; l < 9; ++l)
    mk[l] = *reinterpret_cast<const u32x4*>(frag_ptr(const_cast<void*>(a.acts), tile, a.astride, A_MASK + l, r, h));
#define ZSINK(slot0) PairSink{a.dz, tile0, a.zstride, slot0, Z_LO, r, h}
  ZSINK(L::Z_RGB).put(0, zrh[0], zrl[0]);
  ZSINK(L::Z_A).put(0, zah[0], zal[0]);
  bf16x8 zdh[8], zdl[8];
  layer_bwd<1, 4, true>(ws, L::B_RGB, zrh, zrl, zdh, zdl, mk[8], lane, ZSINK(L::Z_D));
  bf16x8 zxh[16], zxl[16], zyh[16], zyl[16];
  if constexpr (FOLD) {
    bf16x8 cth[9], ctl[9];
#pragma unroll
    for (int k = 0; k < 8; ++k) { cth[k] = zdh[k]; ctl[k] = zdl[k]; }
    cth[8] = zah[0]; ctl[8] = zal[0];
    layer_bwd<9, 8, true>(ws, LF::B_DA, cth, ctl, zyh, zyl, mk[7], lane, ZSINK(L::Z_L0 + 112));   // dZ7
  } else {
    layer_bwd<8, 8, false>(ws, L::B_DIR, zdh, zdl, zxh, zxl, mk[8], lane, ZSINK(L::Z_F));        // d feature
    bf16x8 cth[17], ctl[17];
#pragma unroll
    for (int k = 0; k < 16; ++k) { cth[k] = zxh[k]; ctl[k] = zxl[k]; }
    cth[16] = zah[0]; ctl[16] = zal[0];
    layer_bwd<17, 8, true>(ws, L::B_FA, cth, ctl, zyh, zyl, mk[7], lane, ZSINK(L::Z_L0 + 112));   // dZ7
  }
  constexpr int SH = FOLD ? LF::B_SHIFT : 0;                 // the trunk sits 128 pairs earlier in the folded stream
  layer_bwd<16, 8, true>(ws, L::B_L7 - SH, zyh, zyl, zxh, zxl, mk[6], lane, ZSINK(L::Z_L0 + 96));     // dZ6
  layer_bwd<16, 8, true>(ws, L::B_L6 - SH, zxh, zxl, zyh, zyl, mk[5], lane, ZSINK(L::Z_L0 + 80));     // dZ5
  layer_bwd<16, 8, true>(ws, L::B_L5 - SH, zyh, zyl, zxh, zxl, mk[4], lane, ZSINK(L::Z_L0 + 64));     // dZ4
  layer_bwd<16, 8, true>(ws, L::B_L4 + 0 * 128 - SH, zxh, zxl, zyh, zyl, mk[3], lane, ZSINK(L::Z_L0 + 48));   // dZ3
  layer_bwd<16, 8, true>(ws, L::B_L4 + 1 * 128 - SH, zyh, zyl, zxh, zxl, mk[2], lane, ZSINK(L::Z_L0 + 32));   // dZ2
  layer_bwd<16, 8, true>(ws, L::B_L4 + 2 * 128 - SH, zxh, zxl, zyh, zyl, mk[1], lane, ZSINK(L::Z_L0 + 16));   // dZ1
  layer_bwd<16, 8, true>(ws, L::B_L4 + 3 * 128 - SH, zyh, zyl, zxh, zxl, mk[0], lane, ZSINK(L::Z_L0 + 0));    // dZ0
#undef ZSINK
}

template <bool FOLD>
__global__ void __launch_bounds__(64 * NW) s16_bwd_kernel(BwdArgs a) {
  typedef std::conditional_t<FOLD, BwdRingFold, BwdRing> Ring;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t ntiles = (a.M + 31) >> 5, nsuper = (ntiles + NW - 1) / NW;
  Ring ws;
  ws.wsrc = reinterpret_cast<const char*>(a.wb);
  ws.lane16 = 16 * lane;
  ws.lds0 = __builtin_amdgcn_readfirstlane(lds_addr_of(ring_smem));
  ws.wv = wv;
  ws.start(lane);
  PassQueue pq;                           // dynamic pass queue (mlp_ring.h); a.queue == nullptr: static split
  pq.init(a.queue, ws.lds0 + Ring::BIAS_OFF);
  for (int64_t sp = blockIdx.x; sp < nsuper;) {
    int ln = lane;
    asm volatile("" : "+v"(ln));
    ws.new_pass();
    bwd_tiles<FOLD>(a, ws, sp * NW + wv, ntiles, ln, pq);
    // the pass ends inside the last chunk (2200, folded 1944, is not a multiple of 32): the next pass starts at a chunk boundary again
    // because fragment indices restart at 0
    sp = pq.next(sp);
  }
  ws.drain();
  pq.leave();
}

}  // namespace s16
}  // namespace nerf
