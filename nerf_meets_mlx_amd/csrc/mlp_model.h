// Host-side description of the MLP models that have kernels: resolve() turns a nerf_mlp_arch into everything the C ABI entry
// points of mlp.hip need to know about it -- parameter count, byte offset of every stream in the packed buffer, fragment slots
// per sample tile of the training stores, weight-gradient jobs, and the (slot, fragments) of each layer for the test hook.
// A new model or precision is described HERE; the entry points hold no layout arithmetic of their own.  (Host only: no kernel
// reads any of this; the kernels take the layouts from mlp_layout.h / mlp_arch2.h and the per-precision headers.)  The kernel
// arguments of the image and 2 x 64 models (mlp_input2.h) are filled here too, from the description: img_args / small_args.
#pragma once
#include "mlp_input2.h"
#include "mlp_frag.h"
#include "mlp32.h"
#include "mlp22.h"
#include "mlp_s16.h"
#include "mlp_s16x.h"

namespace nerf {

inline int g_tile_pad16 = 0;     // "tile_pad16": extra 16-byte units between sample tiles of the fragment stores

enum class Shape { View, Image, Small };    // 8x256 (63+27 -> 4) | 8x256 image fitting (40 -> out_ch) | 2x64 hash grid (32+16 -> 4)
// precision of a model = nerf_mlp_arch.precision (ABI 3), nothing process-wide: models of different precision can be packed,
// queried and trained side by side on any streams.
//   Bf16  (16, or 0): bf16 MFMA operands, fp32 accumulate (mlp.hip)
//   F32   (32): the fp32 reference-precision kernels of mlp32.hip (8x256 shapes only); stores in its own row format
//   Split (22): reference tolerance on the 16-bit matrix pipe: split-fp16 inference (mlp22.hip, view model) and split-bf16
//               training (mlp_s16.hip; image / 2x64: mlp_s16x.hip for both).  Such a model carries the bf16 image too and
//               shares its fp32 bias slots.
enum class Prec { Bf16, F32, Split };
// streams of the packed buffer, in buffer order; the split-bf16 stream is mlp_s16.hip's (view) or mlp_s16x.hip's (image, 2x64)
enum Stream { S_FWD, S_BWD, S_BIAS, S_FWD16, S_F32, S_F22, S_S16, S_COUNT };

struct DebugSlot { int slot, nfrag; };      // nfrag 0: the layer does not exist in this store
#define NERF_HIDDEN8(b) {b, 16}, {b + 16, 16}, {b + 32, 16}, {b + 48, 16}, {b + 64, 16}, {b + 80, 16}, {b + 96, 16}, {b + 112, 16}

constexpr DwJob view_pos(int l) { return {L::Z_L0 + 16 * l, 16, L::A_H0 + 16 * (l - 1), 16, L::pw(l), 256, 0, 256, 256, L::pb(l)}; }
constexpr DwJob img_pos(int l) { return {LI::Z_L0 + 16 * l, 16, LI::A_H0 + 16 * (l - 1), 16, LI::pw(l), 256, 0, 256, 256, LI::pb(l)}; }
// {dz_slot, nf, act_slot, kf, w_off, ldw, col0, n_valid, k_valid, b_off}
constexpr DwJob VIEW_JOBS[] = {
    {L::Z_L0, 16, L::A_PE, 4, L::P_W0, 63, 0, 256, 63, L::P_B0},                       // pos0
    view_pos(1), view_pos(2), view_pos(3), view_pos(4),                                // pos1..4
    {L::Z_L0 + 80, 16, L::A_H0 + 64, 16, L::P_W5, 319, 63, 256, 256, L::P_B5},         // pos5 | H4
    {L::Z_L0 + 80, 16, L::A_PE, 4, L::P_W5, 319, 0, 256, 63, -1},                      // pos5 | PE
    view_pos(6), view_pos(7),                                                          // pos6, pos7
    {L::Z_F, 16, L::A_H0 + 112, 16, L::P_WF, 256, 0, 256, 256, L::P_BF},               // feature
    {L::Z_A, 1, L::A_H0 + 112, 16, L::P_WA, 256, 0, 1, 256, L::P_BA},                  // alpha
    {L::Z_D, 8, L::A_FEAT, 16, L::P_WD, 283, 0, 128, 256, L::P_BD},                    // dir0 | feature
    {L::Z_D, 8, L::A_DPE, 2, L::P_WD, 283, 256, 128, 27, -1},                          // dir0 | dirPE
    {L::Z_RGB, 1, L::A_HD, 8, L::P_WR, 128, 0, 3, 128, L::P_BR},                       // rgb
};
// The same gradients with the feature and dir0 layers factored ("dw_factor", precision 22).  feature = W_F h7 + b_F has no
// activation (models/NeRF.py:231), so with  G = dZ_D H7^T (128 x 256)  and  db_D = row sums of dZ_D
//     dW_F = W_D[:, :256]^T G,   db_F = W_D[:, :256]^T db_D,   dW_D[:, :256] = G W_F^T + db_D b_F^T
// and the jobs `feature`, `alpha` and `dir0 | feature` (73 operand fragments per sample tile, H7 read three times) become ONE job
// over the nine adjacent dZ fragments Z_A, Z_D .. Z_D + 7 and H7 (25 fragments): row 0 of its result is d alpha, rows 16 .. 143
// are G (DwJob::aux_row0), which the post step of mlp_dwf.hip multiplies with the packed weights once per call.
static_assert(L::Z_D == L::Z_A + 1, "d alpha and dZ_D are adjacent dZ fragments");
// A FOLDED split-bf16 training image ("train_fold": mlp_s16.h; streams and fp32 copies: mlp_index.h, namespace LF) multiplies with
// W' = W_D[:, :256] W_F in the forward and the chain, so G is exactly dL/dW' there; it ALWAYS runs this list -- the post step then reads
// the fp32 masters from the image's copies --, and its stores have no feature / dZ_F blocks (slots L::A_FEAT, L::Z_F stay unwritten; the
// slot numbering and the strides are unchanged).  mlp.hip: train_folded().
constexpr DwJob VIEW_JOBS_FACTORED[] = {
    VIEW_JOBS[0], VIEW_JOBS[1], VIEW_JOBS[2], VIEW_JOBS[3], VIEW_JOBS[4], VIEW_JOBS[5], VIEW_JOBS[6], VIEW_JOBS[7], VIEW_JOBS[8],
    {L::Z_A, 9, L::A_H0 + 112, 16, L::P_WA, 256, 0, 16 + 128, 256, L::P_BA, 1, 16},    // alpha | G, db_D (shared)
    VIEW_JOBS[12], VIEW_JOBS[13],                                                      // dir0 | dirPE, rgb
};
constexpr DwJob IMG_JOBS[] = {
    {LI::Z_L0, 16, LI::A_X, 3, LI::P_W0, 40, 0, 256, 40, LI::P_B0},                    // pos0
    img_pos(1), img_pos(2), img_pos(3), img_pos(4),                                    // pos1..4
    {LI::Z_L0 + 80, 16, LI::A_H0 + 64, 16, LI::P_W5, 296, 40, 256, 256, LI::P_B5},     // pos5 | H4
    {LI::Z_L0 + 80, 16, LI::A_X, 3, LI::P_W5, 296, 0, 256, 40, -1},                    // pos5 | x
    img_pos(6), img_pos(7),                                                            // pos6, pos7
    {LI::Z_OUT, 1, LI::A_H0 + 112, 16, LI::P_WO, 256, 0, 0, 256, 0},                   // output: n_valid, b_off patched with out_ch
};
constexpr DwJob SMALL_JOBS[] = {
    {LN::Z_L0, 4, LN::A_X, 2, LN::P_W0, 32, 0, 64, 32, LN::P_B0},                      // pos0
    {LN::Z_L1, 4, LN::A_H0, 4, LN::P_W1, 64, 0, 64, 64, LN::P_B1},                     // pos1
    {LN::Z_F, 4, LN::A_H1, 4, LN::P_WF, 64, 0, 64, 64, LN::P_BF},                      // feature
    {LN::Z_A, 1, LN::A_H1, 4, LN::P_WA, 64, 0, 1, 64, LN::P_BA},                       // alpha
    {LN::Z_D, 2, LN::A_FEAT, 4, LN::P_WD, 80, 0, 32, 64, LN::P_BD},                    // dir0 | feature
    {LN::Z_D, 2, LN::A_DX, 1, LN::P_WD, 80, 64, 32, 16, -1},                           // dir0 | direction features
    {LN::Z_RGB, 1, LN::A_HD, 2, LN::P_WR, 32, 0, 3, 32, LN::P_BR},                     // rgb
};

// what is fixed per shape; the streams a precision adds and out_ch are applied by resolve()
struct ShapeInfo {
  int64_t params;                            // image: without the output layer
  int f_frags, b_frags, bias_floats;         // bf16 image: forward | transposed stream (1 KiB fragments) | fp32 bias slots
  int f16_frags;                             // | forward stream of the 16x16x32 inference variant (view model only)
  int64_t split_bytes;                       // split-bf16 streams of a precision-22 model
  int a_slots[2], z_slots[2];                // fragment slots per 32-sample tile of acts / dZ: [0] bf16, [1] split bf16
  int a_lo, z_lo;                            // split-bf16 stores: slot distance from a hi block to its lo block
  const DwJob* jobs; int njobs;
  // test hook, [kind: 0 acts, 1 dZ][layer].  view: pos0..7, 8 feature, 9 dir0, 10 / 11 PE, dirPE (acts) or d alpha, d rgb (dZ);
  // image: pos0..7, acts 10 = input rows (48 = 40 + pad), dZ 8 = output gradient; 2x64: pos0, pos1, 8 feature, 9 dir0,
  // 10 / 11 = position, direction inputs (acts) or d alpha, d rgb (dZ)
  DebugSlot debug[2][12];
};
constexpr ShapeInfo SHAPES[3] = {
    {L::P_TOTAL, L::F_TOTAL, L::B_PADDED, L::BI_TOTAL, L::F16_PADDED, s16::PACKED_BYTES,
     {L::A_SLOTS, s16::A_SLOTS}, {L::Z_SLOTS, s16::Z_SLOTS}, s16::A_LO, s16::Z_LO, VIEW_JOBS, sizeof(VIEW_JOBS) / sizeof(DwJob),
     {{NERF_HIDDEN8(L::A_H0), {L::A_FEAT, 16}, {L::A_HD, 8}, {L::A_PE, 4}, {L::A_DPE, 2}},
      {NERF_HIDDEN8(L::Z_L0), {L::Z_F, 16}, {L::Z_D, 8}, {L::Z_A, 1}, {L::Z_RGB, 1}}}},
    {LI::P_WO, LI::F_TOTAL, LI::B_PADDED, LI::BI_TOTAL, 0, s16x::IMG_PACKED_BYTES,
     {LI::A_SLOTS, s16x::IMG_A_SLOTS}, {LI::Z_SLOTS, s16x::IMG_Z_SLOTS}, s16x::IMG_A_LO, s16x::IMG_Z_LO, IMG_JOBS, sizeof(IMG_JOBS) / sizeof(DwJob),
     {{NERF_HIDDEN8(LI::A_H0), {0, 0}, {0, 0}, {LI::A_X, 3}, {0, 0}},
      {NERF_HIDDEN8(LI::Z_L0), {LI::Z_OUT, 1}, {0, 0}, {0, 0}, {0, 0}}}},
    {LN::P_TOTAL, LN::F_PADDED, LN::B_PADDED, LN::BI_TOTAL, 0, s16x::SM_PACKED_BYTES,
     {LN::A_SLOTS, s16x::SM_A_SLOTS}, {LN::Z_SLOTS, s16x::SM_Z_SLOTS}, s16x::SM_A_LO, s16x::SM_Z_LO, SMALL_JOBS, sizeof(SMALL_JOBS) / sizeof(DwJob),
     {{{LN::A_H0, 4}, {LN::A_H1, 4}, {0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}, {LN::A_FEAT, 4}, {LN::A_HD, 2}, {LN::A_X, 2}, {LN::A_DX, 1}},
      {{LN::Z_L0, 4}, {LN::Z_L1, 4}, {0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}, {LN::Z_F, 4}, {LN::Z_D, 2}, {LN::Z_A, 1}, {LN::Z_RGB, 1}}}},
};
#undef NERF_HIDDEN8

inline int64_t padded_tiles(int64_t M) { return (((M + 31) / 32) + 7) / 8 * 8; }   // 32-sample tiles, whole 8-tile super-tiles

struct Model {
  bool ok = false;                           // false: no HIP kernel for this arch (sizes read -1, the rest is unset)
  Shape shape; Prec prec; int out_ch;
  const ShapeInfo* info;
  int64_t params, packed_bytes;
  int64_t off[S_COUNT];                      // byte offset of each stream in the packed buffer; -1: the model has none
  int a_slots, z_slots;                      // of this precision (unused by Prec::F32)

  bool split() const { return prec == Prec::Split; }
  // the only places that add to a `packed` pointer
  template <class T> const T* stream(const void* packed, Stream s) const { return reinterpret_cast<const T*>(static_cast<const char*>(packed) + off[s]); }
  template <class T> T* stream(void* packed, Stream s) const { return reinterpret_cast<T*>(static_cast<char*>(packed) + off[s]); }
  // tile strides of the fragment stores, in 16-byte units
  int64_t astride() const { return (int64_t)a_slots * 64 + g_tile_pad16; }
  int64_t zstride() const { return (int64_t)z_slots * 64 + g_tile_pad16; }
  // sizes of the training stores of M samples (-1: unsupported arch or M < 0)
  int64_t acts_bytes(int64_t M) const { return !ok || M < 0 ? -1 : prec == Prec::F32 ? f32::acts_bytes(M) : padded_tiles(M) * astride() * 16; }
  // the split-K partial tiles of the weight-gradient kernels live behind the dZ fragment blocks
  int64_t dz_bytes(int64_t M) const {
    return !ok || M < 0 ? -1 : prec == Prec::F32 ? f32::dz_bytes(M) : padded_tiles(M) * zstride() * 16 + DW_PARTIAL_BYTES;
  }
  float* dw_partial(void* dz, int64_t ntiles) const { return reinterpret_cast<float*>(static_cast<char*>(dz) + padded_tiles(ntiles * 32) * zstride() * 16); }
  // copies the weight-gradient jobs whose bit is set in `mask` (0: all) to dst, returns their number.  factored: the view model's
  // precision-22 list with the shared job (VIEW_JOBS_FACTORED; the caller runs the post step behind its reduce).  A mask names
  // jobs of the legacy table, so it keeps that table.
  bool can_factor() const { return shape == Shape::View && prec == Prec::Split; }
  int dw_jobs(DwJob* dst, int mask, bool factored = false) const {
    int nj = 0;
    if (factored && can_factor() && !mask) {
      for (const DwJob& j : VIEW_JOBS_FACTORED) dst[nj++] = j;
      return nj;
    }
    for (int j = 0; j < info->njobs; ++j) {
      if (mask && !((mask >> j) & 1)) continue;
      dst[nj] = info->jobs[j];
      if (shape == Shape::Image && j == info->njobs - 1) { dst[nj].n_valid = out_ch; dst[nj].b_off = LI::P_WO + out_ch * 256; }
      ++nj;
    }
    return nj;
  }
  // (slot, fragments) of `layer` in the activation (kind 0) or dZ (kind 1) store; nfrag 0: none
  DebugSlot debug_slot(int kind, int layer) const {
    return (layer < 0 || layer > 11 || (kind != 0 && kind != 1)) ? DebugSlot{0, 0} : info->debug[kind][layer];
  }
};

inline Model resolve(const nerf_mlp_arch* a) {
  Model m{};
  m.params = m.packed_bytes = -1;
  if (!a) return m;
  if (a->precision != 0 && a->precision != 16 && a->precision != 32 && a->precision != 22) return m;
  m.prec = a->precision == 32 ? Prec::F32 : a->precision == 22 ? Prec::Split : Prec::Bf16;
  if (m.prec == Prec::F32 && !(a->n_layers == 8 && a->width == 256)) return m;   // fp32 MFMA kernels: the 8 x 256 models (view head or image)
  if (a->n_layers == 2 && a->width == 64 && a->skip_layer < 0 && a->use_viewdirs == 1 && a->in_pos == 32 && a->in_dir == 16) m.shape = Shape::Small;
  else if (a->n_layers != 8 || a->width != 256 || a->skip_layer != 4) return m;
  else if (a->use_viewdirs == 1 && a->in_pos == 63 && a->in_dir == 27) m.shape = Shape::View;
  else if (a->use_viewdirs == 0 && a->in_pos == 40 && a->out_ch >= 1 && a->out_ch <= 4) m.shape = Shape::Image;
  else return m;
  const ShapeInfo& s = SHAPES[(int)m.shape];
  m.info = &s;
  m.out_ch = a->out_ch;
  m.params = s.params + (m.shape == Shape::Image ? (int64_t)a->out_ch * 257 : 0);
  m.a_slots = s.a_slots[m.split()]; m.z_slots = s.z_slots[m.split()];
  for (int i = 0; i < S_COUNT; ++i) m.off[i] = -1;
  int64_t end = 0;
  auto put = [&](Stream st, int64_t bytes) { m.off[st] = end; end += bytes; };
  put(S_FWD, (int64_t)s.f_frags * 1024);
  put(S_BWD, (int64_t)s.b_frags * 1024);
  put(S_BIAS, (int64_t)s.bias_floats * 4);
  if (s.f16_frags) put(S_FWD16, (int64_t)s.f16_frags * 1024);
  if (m.prec == Prec::F32) put(S_F32, f32::PACKED_BYTES);
  if (m.split() && m.shape == Shape::View) put(S_F22, f22::PACKED_BYTES);
  if (m.split()) put(S_S16, s.split_bytes);
  m.packed_bytes = end;
  m.ok = true;
  return m;
}

// Kernel arguments of the image / 2 x 64 model in the model's precision: the bf16 streams, or the (hi, lo) pair streams of a
// precision-22 model (forward stream first), the shared fp32 bias slots, the tile strides; everything per call unset.
template <class A>
inline void weight_args(A& a, const Model& m, const void* packed, int split_f_frags) {
  a.wf = m.stream<bf16x8>(packed, m.split() ? S_S16 : S_FWD);
  a.wb = m.split() ? a.wf + (size_t)split_f_frags * 64 : m.stream<bf16x8>(packed, S_BWD);
  a.bias = m.stream<float>(packed, S_BIAS);
  a.astride = m.astride(); a.zstride = m.zstride();
  a.x = nullptr; a.out = nullptr; a.acts = nullptr; a.dz = nullptr; a.M = 0;
}
inline void img_args(ImgArgs& a, const Model& m, const void* packed) {
  weight_args(a, m, packed, s16x::IMG_F_FRAGS);
  a.out_ch = m.out_ch; a.d_out = nullptr;
}
inline void small_args(SmallArgs& a, const Model& m, const void* packed) {
  weight_args(a, m, packed, s16x::SM_F_FRAGS);
  a.d_raw = nullptr; a.d_x = nullptr;
  a.rays = nullptr; a.z = nullptr; a.n = 1; a.tables = nullptr; a.tables_h = nullptr; a.T = 0; a.pos_scale = 1.0f; a.pos_offset = 0.0f;
  a.ray_major = 0; a.B = 0;
  for (int l = 0; l < 32; ++l) { a.rt.res[l] = 0.0f; a.lw.w[l] = 1.0f; }
}

}  // namespace nerf
