/* nerf_hip.h -- C ABI of the MI355X-native NeRF hot path (libnerf_hip.so, gfx950).
 *
 * This is the drop-in boundary of SURVEY.md 8(b).  The reference
 * (piljoong-jeong/nerf_meets_mlx) has no FFI layer of its own: its hot path is a set of
 * Python functions over mlx arrays.  Each entry point below replaces the device work of
 * one (or a fused group) of those functions; the citation after "replaces:" is the
 * reference file:line.  The Python host package `nerf_meets_mlx_amd` binds these with
 * ctypes and re-exports the reference's function names/signatures.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) owned by the caller unless marked "host";
 *     the library allocates nothing.  What a call computes depends only on its arguments: the arithmetic of a
 *     network (bf16 or fp32 MFMA operands) is a field of its `nerf_mlp_arch`, so models of different precision
 *     can be used side by side, on any streams.  Process-wide state is limited to the last error string and the
 *     A/B measurement knobs of nerf_set_option (kernel-variant selection; they never change results' layout,
 *     buffer sizes or which weight image a launch reads).
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, no hidden
 *     synchronisation, safe to capture into a hipGraph.  A captured call freezes every BY-VALUE argument: each replay
 *     reads the device buffers as they are then, but runs with the host values of capture time -- Adam's `lr` and `step`
 *     and the bias-correction factors c1, c2 derived from `step` on the host, the seeds and offsets of the sampling
 *     entries, the level weights (copied into the launch), sizes, flags, and the A/B options of nerf_set_option as they
 *     stood.  The ring kernels' pass-queue slot is frozen too: eager launches take the 256 slots of their translation
 *     unit round-robin, a captured launch keeps its slot for the life of the graph.  Launches on one stream are safe (the
 *     last workgroup clears the slot before the next launch starts); a graph holding ring-kernel launches must not be
 *     replayed CONCURRENTLY with 256 or more later launches of the same unit on other streams -- or capture it with
 *     nerf_set_option("pass_queue", 0), which changes no result.  The host package refuses the captures a replay would
 *     get silently wrong (bias-corrected Adam, optimiser state created inside the capture) and records its lazy
 *     conversions (weight image, fp16 table shadow) into every graph: DESIGN.md "Graph capture".
 *   - tensors are dense row-major float32 unless stated; index tensors are int64.
 *   - return value: 0 = NERF_OK, negative = NERF_E_*;  nerf_last_error() gives text.
 *   - thread-compatible (not thread-safe); one process per GPU.
 */
#ifndef NERF_HIP_H
#define NERF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 2): nerf_mlp_packed_bytes / nerf_mlp_dz_bytes return larger sizes (fp32 weight streams behind the bf16 image;
 * split-K partial tiles behind the dZ blocks) and nerf_mlp_acts_bytes / _dz_bytes depend on "mlp_precision": callers that
 * always size their buffers with these functions are unaffected; new entry points were only added.                  */
/* 3 (round 3): `precision` became a field of nerf_mlp_arch (was the process-global option "mlp_precision"):
 * nerf_mlp_packed_bytes / _acts_bytes / _dz_bytes / _pack and every forward / backward read it from the arch they are
 * given.  The struct grew by one int at the end; a v2 caller must be recompiled.  (Later in round 3, no ABI change: for
 * precision 32 nerf_mlp_acts_bytes counts 64 more rows per 32-sample tile -- the ReLU sign bits the backward chain reads
 * instead of the float32 rows -- and nerf_mlp_dz_bytes 34 MB of split-K partial blocks, so that the fp32 weight gradient
 * is a fixed-order sum like the bf16 one: bit-reproducible, no atomics.)                                           */
#define NERF_ABI_VERSION 3

#define NERF_OK 0
#define NERF_E_NULL (-1)        /* required pointer is NULL                        */
#define NERF_E_SHAPE (-2)       /* size / shape out of the supported range         */
#define NERF_E_UNSUPPORTED (-3) /* architecture / mode not implemented in HIP      */
#define NERF_E_HIP (-4)         /* HIP runtime error (launch failed, bad stream)   */
#define NERF_E_RCCL (-5)        /* RCCL error                                      */

int nerf_abi_version(void);
const char* nerf_last_error(void);

/* ---------------------------------------------------------------- rays (a1, a3, a4)
 * rays are packed exactly like the reference's `rays_linear`
 * (entrypoints/__test_nerf.py:60-82, rendering/render.py:319-328):
 *   [o(3), d(3), near, far, viewdirs(3)] = 11 floats per ray.                        */
#define NERF_RAY_STRIDE 11

/* Distinct pseudo-random indices in [0, domain): out[i] = P_seed(offset + i) where P is a
 * keyed bijection of [0, domain) (4-round Feistel + cycle walking).  Replaces
 * `np.random.choice(H*W, N_rand, replace=False)` entrypoints/__test_nerf.py:229 with O(n)
 * device work; requires offset + n <= domain.  Bit-exact vs the host mirror
 * nerf_meets_mlx_amd.ops.index.pixel_permutation.                                  */
int nerf_pixel_permutation(int64_t* out_idx, int64_t n, int64_t domain, uint64_t seed, uint64_t offset,
                           void* stream);

/* replaces: rendering/ray.py:7-35 get_rays + the (row, col) gather of
 * entrypoints/__test_nerf.py:213-236 + viewdirs/near/far packing (:60-82).
 * pixel_idx: [n] flat row-major pixel indices, or NULL for all H*W pixels in order
 * (then n must equal H*W).  K: host, 9 DOUBLES row-major (the reference's K is a float64 numpy array,
 * entrypoints/__test_nerf.py:170-174); c2w: host, 12 floats (3x4, row-major).  Directions are
 * evaluated in float64 and rounded once to float32.
 * coords (optional, may be NULL): [n,2] int64 (row, col) = (idx / W, idx % W).        */
int nerf_ray_gen(const int64_t* pixel_idx, int64_t n, int H, int W, const double* K_host, const float* c2w_host,
                 float near, float far, float* rays, int64_t* coords, void* stream);

/* replaces, for the training step, the three calls around it as ONE launch: entrypoints/__test_nerf.py:213-236 (N_rand
 * distinct pixels of one image, their rays, their target colours) + :60-82 (ray packing).  Pixel i of the batch is
 * P(seed; offset + i) of nerf_pixel_permutation over H*W; rays [n,11] as nerf_ray_gen; target [n,3] = image[pixel];
 * pixel_idx (optional) [n] int64.  image: [H*W,3] float32 device.  Outputs bit-identical to the three separate calls. */
int nerf_sample_batch(int64_t n, int H, int W, uint64_t seed, uint64_t offset, const double* K_host, const float* c2w_host,
                      float near, float far, const float* image, float* rays, float* target, int64_t* pixel_idx,
                      void* stream);

/* nerf_sample_batch for a straight RGBA image ("background colour" below): image [H*W, 4], target [n, 4] = image[pixel], both
 * 16-byte aligned (NERF_E_SHAPE otherwise).  Pixels, rays and pixel_idx are those of nerf_sample_batch with the same arguments,
 * bit for bit.  Additive: NERF_ABI_VERSION stays 3.                                                                            */
int nerf_sample_batch_rgba(int64_t n, int H, int W, uint64_t seed, uint64_t offset, const double* K_host, const float* c2w_host,
                           float near, float far, const float* image, float* rays, float* target, int64_t* pixel_idx,
                           void* stream);

/* out[i, :] = src[idx[i], :]   (target pixel gather, entrypoints/__test_nerf.py:236).
 * idx[i] outside [0, n_src) is never dereferenced: that output row is NaN.               */
int nerf_gather_rows(const float* src, int64_t n_src, const int64_t* idx, int64_t n, int channels, float* out,
                     void* stream);

/* replaces: rendering/ray.py:39-70 ndc_rays (in place on the o,d columns of `rays`)    */
int nerf_ndc_rays(float* rays, int64_t n, int H, int W, float focal, float near, void* stream);

/* ---------------------------------------------------------------- sampling (a5-a7, a15, a17)
 * replaces: sampling/uniform.py:7-18, sampling/linear_disparity.py:8-19 (literal),
 * sampling/__init__.py:10-31 add_noise_z (intended semantics).
 * t_rand: [B,n] uniforms in [0,1) (caller's RNG), may be NULL when perturb <= 0.       */
int nerf_sample_coarse(const float* rays, int64_t B, int n, int lindisp, float perturb, const float* t_rand,
                       float* z, void* stream);

/* replaces: sampling/__init__.py:10-31 add_noise_z on caller-supplied depths (the fused form above covers the render
 * path): mids = (z[k] + z[k+1]) / 2, lower = [z_first, mids], upper = [mids, z_last],
 * z_out = lower + (upper - lower) * (t_rand * strength).  z_in, t_rand, z_out: [B,n]; not in place.                */
int nerf_add_noise_z(const float* z_in, const float* t_rand, int64_t B, int n, float strength, float* z_out,
                     void* stream);

/* replaces: sampling/__init__.py:101-177 sample_from_inverse_cdf_torch (u passed in
 * instead of torch.rand) and the sort of entrypoints/__test_nerf.py:288 /
 * rendering/render.py:225.  weights: [B,n] (the reference's [B,n,1] squeezed).
 * Outputs (each may be NULL): z_new [B,N]; z_merged [B,n+N]; cdf [B,n+1];
 * inds [B,N] int64 = searchsorted(cdf, u, side="right") -- bit-exact given (cdf,u) for a monotone cdf (NaN or
 * negative weights give a cdf that is not: inds is then what the binary search finds; a NaN u gives n + 1).
 * z_merged is the exact multiset of the n coarse and the N new depths, ascending, equal depths coarse-first, NaN last
 * -- for any coarse list (ascending or not, with ties, NaN or infinite depths) and for NaN new depths (an infinite
 * first / last coarse depth makes the mid points infinite and their difference NaN).
 * Limits: 2 <= n <= 256, 1 <= N <= 512, n+N <= 768.                                   */
int nerf_importance_sample(const float* z, const float* weights, const float* u, int64_t B, int n, int N, float eps,
                           float* z_new, float* z_merged, float* cdf, int64_t* inds, void* stream);

/* ---------------------------------------------------------------- encodings (a9, a10, a22, a23)
 * replaces: models/embedding.py:23-90 Embedder.embed: [x, sin(f0 x), cos(f0 x), ...];
 * freq_mode 0 = k^2 (reference quirk Q4), 1 = 2^k.  out: [M, D*(1+2*n_freqs)].        */
int nerf_encode_freq(const float* x, int64_t M, int D, int n_freqs, int freq_mode, float* out, void* stream);

/* replaces: encoding/sinusoidal.py:39-66: sin([s, s+pi/2]), s = x[...,None]*freq flattened
 * dim-major/freq-minor; optional raw input appended at the end.  freqs: host float[n_freqs]
 * (= 2^linspace(min_exp,max_exp,n), evaluated by the caller so that host and oracle
 * share the table bit for bit; n_freqs <= 32).  out [M, 2*D*n_freqs (+D)].              */
int nerf_encode_sinusoidal(const float* x, int64_t M, int D, int n_freqs, const float* freqs_host,
                           int include_input, float* out, void* stream);

/* replaces: encoding/spherical_harmonics.py:33-94; out [M,(degree+1)^2], 0<=degree<=4  */
int nerf_sh_encode(const float* dirs, int64_t M, int degree, float* out, void* stream);

/* replaces: encoding/multi_hash.py:61-136 (intended semantics).
 * tables [L,T,F] float32, T = 2^log2_T, F in {1,2,4,8}; resolutions: host int[L];
 * out [M, L*F].  backward: d_tables += scatter of d_out (float atomics).              */
int nerf_hashgrid_forward(const float* x, int64_t M, const float* tables, int L, int log2_T, int F,
                          const int* resolutions_host, float* out, void* stream);
int nerf_hashgrid_backward(const float* x, int64_t M, const float* d_out, int L, int log2_T, int F,
                           const int* resolutions_host, float* d_tables, void* stream);

/* One input row per sample for the hash-grid model (BASELINE configs[4]; engine glue the reference never wrote):
 * x_out [B n, L F + (sh_degree+1)^2] = [ hash features of o + z d | SH of the ray's view direction ], i.e.
 * MultiHashEncoding(pts) and SphericalHarmonicsEncoding(viewdirs) of encoding/{multi_hash,spherical_harmonics}.py
 * written side by side; pts_out [B n, 3] (or NULL) keeps the positions for nerf_hashgrid_backward.  The grid sees
 * (o + z d) * pos_scale + pos_offset: the affine map of the scene box onto [0,1]^3 (1, 0 = world coordinates).    */
int nerf_ngp_encode(const float* rays, const float* z, int64_t B, int n, const float* tables, int L, int log2_T,
                    int F, const int* resolutions_host, int sh_degree, float pos_scale, float pos_offset, float* x_out,
                    float* pts_out, void* stream);
/* table gradient with the sample positions taken from rays / depths (o + z d) instead of a point list          */
int nerf_hashgrid_backward_rays(const float* rays, const float* z, int64_t B, int n, const float* d_out, int L,
                                int log2_T, int F, const int* resolutions_host, float pos_scale, float pos_offset,
                                float* d_tables, void* stream);

/* The same for levels [level_lo, level_hi) only (the launches of disjoint level groups can be followed one by one by the
 * all-reduce of their slice of d_tables on another stream), and optionally DETERMINISTIC: fixed_point = 1 makes d_tables
 * an int64 [L,T,F] array of 2^-52 fixed-point accumulators added with integer atomics (associative: the result does not
 * depend on the order the memory side serves the requests; float atomics do).  nerf_adam_step_ex consumes either form.
 * Range of the fixed-point form: an addend with |v| > 256 saturates to +-1.5 x 2^60 units (+-384), a NaN / Inf addend adds
 * 2^61 units, and nerf_adam_step_ex reads an accumulator as a NaN gradient exactly when it lies outside the open window
 * (-2^60, 2^60) units (+-256).  The int64 accumulators wrap: an entry with k saturated addends of sign s, j NaN / Inf addends
 * and an ordinary sum g (units of 2^-52, also summed over ranks) holds k s 1.5 2^60 + j 2^61 + g 2^52 mod 2^64 and reads FINITE
 * whenever that lands inside the window -- e.g. k = 11, 21 or 0 (mod 32) with small g (+128 + g, -128 + g, g), j = 0 (mod 8),
 * or g within 256 of a multiple of +-4096.  Otherwise a diverged run surfaces as NaN parameters, as with float atomics.
 * (Two saturated addends of opposite sign on one entry cancel, like two float gradients of +-1e9 would.) */
int nerf_hashgrid_backward_ex(const float* x, int64_t M, const float* d_out, int L, int log2_T, int F,
                              const int* resolutions_host, int level_lo, int level_hi, int fixed_point, void* d_tables,
                              void* stream);
int nerf_hashgrid_backward_rays_ex(const float* rays, const float* z, int64_t B, int n, const float* d_out, int L,
                                   int log2_T, int F, const int* resolutions_host, float pos_scale, float pos_offset,
                                   int level_lo, int level_hi, int fixed_point, void* d_tables, void* stream);

/* Level weights (coarse-to-fine training of the hash grid: FreeNeRF's frequency mask, Neuralangelo's progressive levels).
 * The `_lw` entries take a per-level weight vector w[L]: float32, each finite and in [0, 1], a HOST array like
 * resolutions_host; NULL means all ones and runs exactly the kernels of the entry without the suffix.  A value outside
 * [0, 1] or a NaN is NERF_E_SHAPE.  Everything else is the argument list of the entry without the suffix.  Each entry
 * without the suffix IS its `_lw` entry called with NULL weights, under its own name in nerf_last_error().
 *   forward         feature (l, f) = w[l] * interp_l,f: ONE float32 multiply after the interpolation above, before any
 *                   rounding to bf16 / fp16 fragments.  w[l] == 0: level l's tables are NOT READ and its features are
 *                   exactly +0, whatever the tables hold (NaN and Inf included).  w[l] == 1: bit-identical to the entry
 *                   without the suffix.
 *   table gradient  g = w[l] * d_out[., l, f] (one float32 multiply), then the addend formula above with g in place of
 *                   d_out.  w[l] == 0: level l issues no atomics and its accumulators are not touched (the LDS
 *                   write-combining path of the coarse levels included).
 *   MLP input gradient: the d_x of nerf_mlp_backward_inputs is unchanged; the weight applies on the way into the tables. */
int nerf_hashgrid_forward_lw(const float* x, int64_t M, const float* tables, int L, int log2_T, int F,
                             const int* resolutions_host, const float* level_weights_host, float* out, void* stream);
int nerf_ngp_encode_lw(const float* rays, const float* z, int64_t B, int n, const float* tables, int L, int log2_T,
                       int F, const int* resolutions_host, const float* level_weights_host, int sh_degree,
                       float pos_scale, float pos_offset, float* x_out, float* pts_out, void* stream);
int nerf_hashgrid_backward_ex_lw(const float* x, int64_t M, const float* d_out, int L, int log2_T, int F,
                                 const int* resolutions_host, const float* level_weights_host, int level_lo,
                                 int level_hi, int fixed_point, void* d_tables, void* stream);
int nerf_hashgrid_backward_rays_ex_lw(const float* rays, const float* z, int64_t B, int n, const float* d_out, int L,
                                      int log2_T, int F, const int* resolutions_host, const float* level_weights_host,
                                      float pos_scale, float pos_offset, int level_lo, int level_hi, int fixed_point,
                                      void* d_tables, void* stream);

/* ---------------------------------------------------------------- compositing (a13)
 * replaces: rendering/render.py:20-96 raw2outputs.  raw [B,n,4] = [rgb, sigma];
 * noise [B,n] (N(0,1), caller's RNG) may be NULL when raw_noise_std == 0.
 * Outputs: rgb [B,3], disp [B], acc [B], weights [B,n], depth [B] (any may be NULL
 * except rgb).  One wavefront per ray, n <= 1024.                                      */
int nerf_composite_forward(const float* raw, const float* z, const float* rays, int64_t B, int n,
                           float raw_noise_std, const float* noise, int white_bkgd, float* rgb, float* disp,
                           float* acc, float* weights, float* depth, void* stream);

/* adjoint of the above (what mlx autograd computes for entrypoints/__test_nerf.py:132,142).
 * d_rgb [B,3] required; d_acc [B], d_depth [B] optional (NULL = 0).  d_raw [B,n,4].     */
int nerf_composite_backward(const float* raw, const float* z, const float* rays, int64_t B, int n,
                            float raw_noise_std, const float* noise, int white_bkgd, const float* d_rgb,
                            const float* d_acc, const float* d_depth, float* d_raw, void* stream);

/* replaces: ops/metric.py:12-14 MSE and its gradient: loss_out[0] += sum((pred-target)^2)
 * / count (caller zeroes it; the workgroups' terms are added atomically, so the last bits depend on their order),
 * d_pred = grad_scale * 2 (pred-target) / count.  loss_out and d_pred may each be NULL; count > 0.       */
int nerf_mse_loss_grad(const float* pred, const float* target, int64_t count, float grad_scale, float* loss_out,
                       float* d_pred, void* stream);

/* replaces, for the training step, the three calls above as ONE pass per ray: what nn.value_and_grad differentiates
 * in entrypoints/__test_nerf.py:47-126 -- raw2outputs (raw_noise_std = 0 there: SURVEY Q5), loss = mean((rgb - target)^2)
 * over B x 3, d_raw = d loss / d raw x grad_scale.  loss_out[0] += loss (caller zeroes it); rgb (optional): [B,3].
 * rgb and d_raw are bit-identical to nerf_composite_forward + nerf_mse_loss_grad + nerf_composite_backward.        */
int nerf_composite_mse_backward(const float* raw, const float* z, const float* rays, int64_t B, int n, int white_bkgd,
                                const float* target, float grad_scale, float* loss_out, float* rgb, float* d_raw,
                                void* stream);

/* replaces: ops/metric.py:20-64 SSIM (unfinished upstream: the body stops after the five windowed moments; this is
 * the formula those moments feed).  pred, gt: [N,C,H,W] float32 device; window_host: the 1-D window (w_size <= 33
 * taps, the 2-D window of create_window :49-55 is its outer product), applied as a depthwise VALID convolution
 * (padding = NO_PAD, :33-42).  sums: [N,2] float64 device, overwritten with
 *   sums[n][0] = sum over (c, y, x) of ((2 mu_p mu_g + c1)(2 s_pg + c2)) / ((mu_p^2 + mu_g^2 + c1)(s_p^2 + s_g^2 + c2))
 *   sums[n][1] = sum of the contrast-structure term (2 s_pg + c2) / (s_p^2 + s_g^2 + c2)
 * over the C (H-w+1)(W-w+1) window positions of image n; the caller divides by that count.
 * c1 = (0.01 L)^2, c2 = (0.03 L)^2 with the dynamic range L of :24-28 are computed by the caller.                 */
int nerf_ssim_sums(const float* pred, const float* gt, int N, int C, int H, int W, const float* window_host,
                   int w_size, float c1, float c2, double* sums, void* stream);

/* ---------------------------------------------------------------- the MLP (a11, a12)
 * replaces: models/NeRF.py:160-243 (NeRF.__init__/forward), :10-48 (run_model),
 * models/embedding.py:4-21 (embed) for the architecture n_layers=8, width=256,
 * skips=[4], use_viewdirs, in_pos=63, in_dir=27, and for the no-view-direction model of the reference's image
 * fitting (entrypoints/__viser_image_learning.py:203-208: in_pos=40, in_dir=0, use_viewdirs=0, out_ch<=4; layers
 * pos0 [256x40] pos1..4 pos5 [256x296] pos6 pos7 output [out_ch x 256]).  Anything else: NERF_E_UNSUPPORTED.
 *
 * Parameter layout (float32, flat, `nerf_mlp_param_count` = 595844 elements), each
 * layer as weight[out][in] row-major followed by bias[out]  (nn.Linear: x @ W^T + b):
 *   pos0 [256x63] pos1..pos4 [256x256] pos5 [256x319] pos6 pos7 [256x256]
 *   feature [256x256]  alpha [1x256]  dir0 [128x283]  rgb [3x128]
 * Gradients use the same layout.  Three instances of the class have kernels: the view
 * model above, the image model {8, 256, 40, 0, 4, 0, out_ch <= 4}
 * (entrypoints/__viser_image_learning.py:198-208) and the Instant-NGP-sized view model
 * {2, 64, 32, 16, -1, 1}: pos0 [64x32] pos1 [64x64] feature [64x64] alpha [1x64]
 * dir0 [32x80] rgb [3x32] = 13 188 parameters (forward / forward_train / backward on
 * embedded rows; no fused positional-encoding query).                                  */
typedef struct nerf_mlp_arch {
  int n_layers;     /* 8   */
  int width;        /* 256 */
  int in_pos;       /* 63  */
  int in_dir;       /* 27  */
  int skip_layer;   /* 4   */
  int use_viewdirs; /* 1   */
  int out_ch;       /* outputs of `output_linear` when use_viewdirs == 0 (models/NeRF.py:196-197); ignored otherwise */
  int precision;    /* 0 or 16: bf16 MFMA operands, fp32 accumulate -- the benchmarked mode (BASELINE configs[1-3]);
                     * 32: the reference's own arithmetic (models/NeRF.py:201-243 runs in MLX float32): float32 operands
                     * on v_mfma_f32_32x32x2_f32, sinf / cosf encodings; 8 x 256 view model only.  Read by
                     * nerf_mlp_packed_bytes / nerf_mlp_pack (an fp32 model's image carries the fp32 weight streams behind
                     * the bf16 one), nerf_mlp_acts_bytes / nerf_mlp_dz_bytes (fp32 stores are larger) and every launch:
                     * use ONE arch value per model for all of them.
                     * 22 (round 4): the reference's float32 TOLERANCE on the 16-bit matrix pipe.  Calls that keep no
                     * activations (nerf_mlp_forward, nerf_query_fused / nerf_render_rays_fused with acts == NULL) run the
                     * split-fp16 kernel of csrc/mlp22.hip: every float32 operand x = hi + lo 2^-11 as two fp16 numbers
                     * (22 significand bits), a product = hi hi + 2^-11 (hi lo + lo hi) on v_mfma_f32_16x16x32_f16 with
                     * fp32 accumulate, encodings within 6e-7 of the float64 sine.  RANGE of the split-fp16 kernel: both
                     * operand kinds, weights and layer inputs (activations, encodings), live in fp16's exponent range.
                     *   High end: |w| and |activation| must stay <= 65504.  The conversions overflow (nothing saturates): a
                     *     larger operand becomes inf, its lo part NaN, and every output that depends on it is inf / NaN --
                     *     never a silent wrong value.
                     *   Low end: a weight below 2^-14 goes to the lo part whole and carries 11 significand bits, not 22
                     *     (absolute error <= 2^-26); an activation below 2^-14 has a subnormal hi part, which the
                     *     conversion and the matrix unit keep (absolute error <= 2^-36).  Nothing is flushed to zero.
                     *   Window: the 1e-4 forward tolerance is promised while the hidden layers' activation scales, and with
                     *     them the weights, stay within a factor 2^7 either way of the unit operating point (weights of
                     *     order 1 / sqrt(fan-in), activations of order 1): measured <= 7e-6 of the output scale there.  Up
                     *     to 2^14 either way every output is finite and the error grows to 3.5e-4 (the 11-bit small
                     *     weights); from 2^15 upwards activations overflow.  tests/test_gpu_range.py holds the kernel to
                     *     a CPU emulation of these formats over that whole range (DESIGN.md "Operand range").
                     *   The other MLP paths -- split bf16 (below), bf16 (precision 16) and fp32 (precision 32) -- carry
                     *     float32's exponent range and are exponent-shift invariant: rescaling the hidden layers by exact
                     *     powers of two (2^-20 .. 2^20 tested) changes no bit of the forward output, no ReLU decision and,
                     *     mapped back through the same powers of two, no bit of the gradients.
                     * Everything that keeps activations (training forward with acts != NULL, nerf_mlp_backward) runs the
                     * split-bf16 kernels of csrc/mlp_s16.hip: x = hi + lo as two bf16 numbers (16 significand bits at
                     * float32's exponent range -- gradients do not fit fp16's), a product = hi hi + hi lo + lo hi on
                     * v_mfma_f32_32x32x16_bf16 into one fp32 accumulator; hi and lo fragment blocks in the acts / dz
                     * workspaces (twice the bf16 sizes).  Measured against the fp32 oracle: forward <= 1e-5 of the
                     * output scale, dW / db <= 3e-5 rel-L2 per tensor on equal ReLU decisions.  The image carries the
                     * bf16 streams (their fp32 bias slots are shared), the split-fp16 and the split-bf16 streams. */
} nerf_mlp_arch;

int64_t nerf_mlp_param_count(const nerf_mlp_arch* arch);
/* bytes of the packed bf16 MFMA-fragment image of the weights (forward + transposed
 * backward images + fp32 biases) that the kernels stream; rebuilt after every update.   */
int64_t nerf_mlp_packed_bytes(const nerf_mlp_arch* arch);
int nerf_mlp_pack(const nerf_mlp_arch* arch, const float* params, void* packed, void* stream);

/* bytes of the activation / gradient-activation stores for M samples (training only)    */
int64_t nerf_mlp_acts_bytes(const nerf_mlp_arch* arch, int64_t M);
int64_t nerf_mlp_dz_bytes(const nerf_mlp_arch* arch, int64_t M);

/* NeRF.forward(x): x [M, in_pos+in_dir] already embedded -> out [M,4] = [rgb, alpha] raw (view model) or
 * [M,out_ch] (image model).  The _train form also keeps the activations for nerf_mlp_backward.              */
int nerf_mlp_forward(const nerf_mlp_arch* arch, const void* packed, const float* x, int64_t M, float* out,
                     void* stream);
int nerf_mlp_forward_train(const nerf_mlp_arch* arch, const void* packed, const float* x, int64_t M, float* out,
                           void* acts, void* stream);

/* network_query_fn(pts, viewdirs, model) fused with pts = o + z d and both positional
 * encodings (models/NeRF.py:75-80 + rendering/render.py:142,226): rays [B,11], z [B,n]
 * -> raw [B,n,4].  freq_mode as nerf_encode_freq.  acts: NULL for inference, or a
 * buffer of nerf_mlp_acts_bytes(B*n) that keeps the per-layer bf16 activations for
 * nerf_mlp_backward.                                                                    */
int nerf_query_fused(const nerf_mlp_arch* arch, const void* packed, const float* rays, const float* z, int64_t B,
                     int n, int freq_mode, float* raw, void* acts, void* stream);

/* Backward of nerf_query_fused w.r.t. the parameters (the reference gets this from
 * mlx autograd: entrypoints/__test_nerf.py:132,142).  d_raw [M,4]; acts from the forward;
 * dz: scratch of nerf_mlp_dz_bytes(M); grads [param_count] is OVERWRITTEN.              */
int nerf_mlp_backward(const nerf_mlp_arch* arch, const void* packed, const void* acts, const float* d_raw,
                      int64_t M, void* dz, float* grads, void* stream);
/* Same, and dL/d(position features) d_x [M, in_pos] for a trainable encoder in front of the network (the hash
 * grid: nerf_hashgrid_backward takes it).  Only for the Instant-NGP-sized instance of the reference's NeRF class
 * {n_layers 2, width 64, in_pos 32, in_dir 16, skip_layer -1, use_viewdirs 1} (BASELINE configs[4]); the 8 x 256
 * models sit behind fixed encodings and return NERF_E_UNSUPPORTED.                                             */
int nerf_mlp_backward_inputs(const nerf_mlp_arch* arch, const void* packed, const void* acts, const float* d_raw,
                             int64_t M, void* dz, float* grads, float* d_x, void* stream);

/* Test hook (no reference counterpart): one layer of the training stores of the last nerf_query_fused(acts != NULL)
 * / nerf_mlp_backward call, decoded from the fragment-block layout to row-major float32 out[M, width], so that the
 * parity tests can compare EVERY layer's activation and dZ with the oracle (and feed the kernel's own ReLU decisions
 * to the oracle's backward).  8 x 256 view model only.
 *   kind 0 (store = acts): layer 0..7 = relu(pos_l) (models/NeRF.py:221-222), 8 = feature (:231), 9 = relu(dir0)
 *                          (:235-236), 10 = position encoding (64 = 63 + pad), 11 = direction encoding (32 = 27 + pad)
 *   kind 1 (store = dz):   layer 0..7 = dL/d(pre-activation of pos_l), 8 = d feature, 9 = d dir0 pre-activation,
 *                          10 = d alpha (column 0), 11 = d rgb (columns 0..2)
 * nerf_mlp_debug_width returns `width` (16 x fragments) or -1.                                                     */
int nerf_mlp_debug_width(const nerf_mlp_arch* arch, int kind, int layer);
int nerf_mlp_debug_read(const nerf_mlp_arch* arch, const void* store, int kind, int layer, int64_t M, float* out,
                        void* stream);

/* The same rows never leaving the chip: hash gathers + SH evaluated inside the 2 x 64 forward kernel (L = 16, F = 2,
 * sh_degree = 3; arch = {2, 64, 32, 16, -1, 1}) -> raw [B,n,4]; acts as in nerf_query_fused.  The table gradient of
 * such a query takes the sample positions from the rays again: nerf_hashgrid_backward_rays(d_out = the d_x of
 * nerf_mlp_backward_inputs).                                                                                  */
int nerf_ngp_query_fused(const nerf_mlp_arch* arch, const void* packed, const float* rays, const float* z, int64_t B,
                         int n, const float* tables, int L, int log2_T, int F, const int* resolutions_host,
                         int sh_degree, float pos_scale, float pos_offset, float* raw, void* acts, void* stream);
/* Round 4: the same query gathering from an fp16 SHADOW image of the tables (tables_half: [L,T] packed pairs of fp16, 4
 * bytes per entry instead of the 8 of the float32 master pair; NULL = gather `tables`) -- SURVEY 8(d) budgets 512 B of
 * gathers per sample, the float32 pairs are 1024.  Interpolation stays float32.  The shadow is written by
 * nerf_adam_step_shadow in the pass that updates the float32 master tables (encoding/multi_hash.py:79-136 keeps one
 * float32 table; the shadow is this library's, like the packed weight image of the MLPs).                         */
int nerf_ngp_query_fused_h(const nerf_mlp_arch* arch, const void* packed, const float* rays, const float* z, int64_t B,
                           int n, const float* tables, const void* tables_half, int L, int log2_T, int F,
                           const int* resolutions_host, int sh_degree, float pos_scale, float pos_offset, float* raw,
                           void* acts, void* stream);
/* The same query with level weights ("Level weights" above): both fused kernels (bf16 with float32 or fp16-shadow gathers,
 * split-bf16 at precision 22), both store modes, the ray-major inference tiling.  A lane's gathers of a level with
 * w[l] == 0 are predicated off.  level_weights_host == NULL: nerf_ngp_query_fused_h.                                  */
int nerf_ngp_query_fused_lw(const nerf_mlp_arch* arch, const void* packed, const float* rays, const float* z, int64_t B,
                            int n, const float* tables, const void* tables_half, int L, int log2_T, int F,
                            const int* resolutions_host, const float* level_weights_host, int sh_degree, float pos_scale,
                            float pos_offset, float* raw, void* acts, void* stream);

/* ---------------------------------------------------------------- occupancy grid (no reference counterpart)
 * Empty-space skipping for the hash-grid model: Instant-NGP's occupancy grid (Mueller et al. 2022, "Instant Neural Graphics
 * Primitives with a Multiresolution Hash Encoding", section 4), one cascade.  Additive: NERF_ABI_VERSION stays 3.
 *   grid      R^3 cells, R = 2^log2_res (2 <= log2_res <= 10; the model uses 128), over the unit cube the hash grid sees: a position p
 *             maps to u = p * pos_scale + pos_offset (the roundings of nerf_ngp_query_fused_h) and lies in cell
 *             (ix, iy, iz) = floor(u R) per axis, linear index c = ix + R (iy + R iz).  A u outside [0, 1)^3 (NaN included) is in
 *             no cell: always empty.
 *   density   float32 [R^3], indexed by c.
 *   bits      uint32 [R^3 / 32]: cell c is occupied when bit (c & 31) of word c >> 5 is set.
 * Update (engine/occupancy.py drives it): nerf_occ_points -> nerf_ngp_query_fused_h(B = count, n = 1) -> nerf_occ_merge, over all
 * cells, then nerf_occ_finalize.  Cull of a batch: nerf_occ_cull -> query of the K kept rows -> nerf_scatter_rows of raw back.   */

/* One jittered point per cell of [cell0, cell0 + count): rays_out [count, 11] = [p, 0, 0, 0, 0, 0, 0, 0, 0] and z_out [count] = 0,
 * so that the fused query with n = 1 evaluates the field at p.  The jitter is a counter-based stream keyed by (seed, update): the
 * same arguments give the same points on any device or rank.  p always maps back into its own cell (a jittered point the round
 * trip would move out of it is replaced by the cell centre).                                                               */
int nerf_occ_points(int log2_res, int64_t cell0, int64_t count, uint64_t seed, uint64_t update, float pos_scale,
                    float pos_offset, float* rays_out, float* z_out, void* stream);
/* density[i] = max(density[i] * decay, relu(raw[i, 3])) for i < count (raw [count, 4]: sigma is column 3; a NaN sigma counts
 * as 0).  Pass density + cell0 for a slice of the grid.                                                                     */
int nerf_occ_merge(float* density, const float* raw, int64_t count, float decay, void* stream);
/* thr = min(thr_cap, mean(density)) with the mean a fixed-order double sum (bit-reproducible), *thr_out = thr (may be NULL),
 * bits = density > thr.  workspace: nerf_occ_finalize_workspace_bytes(log2_res) bytes of scratch.                           */
int64_t nerf_occ_finalize_workspace_bytes(int log2_res);
int nerf_occ_finalize(const float* density, int log2_res, float thr_cap, void* workspace, float* thr_out, uint32_t* bits,
                      void* stream);
/* Stable ray-major compaction of the samples (ray b, depth j) -> s = b n + j of rays [B, 11] / z [B, n] whose position
 * o + z d lies in an occupied cell: idx_out [K] = the kept s in increasing order, rays_out [K, 11] / z_out [K] their ray rows
 * and depths (a B = K, n = 1 batch for the fused query, nerf_mlp_backward_inputs and nerf_hashgrid_backward_rays_ex), and
 * *count_out = K (device int64).  The three outputs need room for B n rows; K is known on the device only.  raw_fill
 * [B, n, 4] (16-byte aligned, or NULL): the rows of the culled samples are set to (0, 0, 0, 0) in the same pass, the kept rows
 * are not touched.  Block scans, no atomics.  workspace: nerf_occ_cull_workspace_bytes(B, n) bytes of scratch.            */
int64_t nerf_occ_cull_workspace_bytes(int64_t B, int n);
int nerf_occ_cull(const float* rays, const float* z, int64_t B, int n, const uint32_t* bits, int log2_res, float pos_scale,
                  float pos_offset, void* workspace, int64_t* idx_out, int64_t* count_out, float* rays_out, float* z_out,
                  float* raw_fill, void* stream);
/* dst[idx[i], :] = src[i, :] for i < n (the inverse of nerf_gather_rows); an idx[i] outside [0, n_dst) is skipped.          */
int nerf_scatter_rows(const float* src, const int64_t* idx, int64_t n, int channels, float* dst, int64_t n_dst, void* stream);

/* ---------------------------------------------------------------- occupancy-guided ray march (no reference counterpart)
 * Instant-NGP's sampler (Mueller et al. 2022, section 4): every ray is marched at a fixed small step through the scene box, and
 * only the steps that land in occupied cells of the grid above become samples, packed ray by ray.  Additive: NERF_ABI_VERSION
 * stays 3.  All float32, one rounding per operation, in this order (tests/_march_ref.py reproduces every depth and every keep
 * decision bit for bit):
 *   box       lo = (0 - pos_offset) / pos_scale, hi = (1 - pos_offset) / pos_scale (world units; the unit cube of the grid).
 *   step      step_world = s_u * 2 bound with s_u = sqrt(3) / march_steps (1 <= march_steps <= NERF_MARCH_MAX_STEPS); the host
 *             computes it in double and rounds once.  dt = step_world / float(sqrt_double((d0 d0 + d1 d1) + d2 d2)).
 *   interval  t0 = near, t1 = far; per axis a = 0, 1, 2: ta = (lo - o_a) / d_a, tb = (hi - o_a) / d_a,
 *             t0 = fmaxf(t0, fminf(ta, tb)), t1 = fminf(t1, fmaxf(ta, tb)).
 *   no sample a ray with a non-finite o, d, near, far or jitter, a zero component of d, or not (t0 < t1 and dt > 0).
 *   candidates z_k = t0 + ((float)k + j) * dt for k = 0, 1, ... while z_k < t1 and k < 2 march_steps (never binding: the chord of
 *             the box is at most sqrt(3) 2 bound = march_steps step_world long).  j in [0, 1): the ray's jitter.
 *   keep      z_k is kept when its cell (the roundings of nerf_occ_cull) exists and is occupied; with bits == NULL (the warm-up)
 *             when its cell exists.  At most march_steps samples are kept per ray, the nearest first.
 * Output, one B = K, n = 1 batch for nerf_ngp_query_fused_h / nerf_mlp_backward_inputs / nerf_hashgrid_backward_rays_ex:
 * offsets int64 [B + 1] (ray b owns [offsets[b], offsets[b + 1]), offsets[B] = K), rows_out [K, 11] (copies of the ray's row),
 * z_out [K].  Two calls: nerf_occ_march_count writes offsets[B] = K only (the caller reads K and sizes rows_out / z_out), then
 * nerf_occ_march_write, with the same arguments and workspace, writes offsets[0 .. B - 1] and the samples.  Count -> block scan
 * -> write, no atomics: every output is bit-reproducible.  jitter: float32 [B], or NULL for jitter_const on every ray.
 * workspace: nerf_occ_march_workspace_bytes(B) bytes, kept between the two calls.                                         */
#define NERF_MARCH_MAX_STEPS 1024
int64_t nerf_occ_march_workspace_bytes(int64_t B);
int nerf_occ_march_count(const float* rays, int64_t B, const float* jitter, float jitter_const, const uint32_t* bits, int log2_res,
                         float pos_scale, float pos_offset, float step_world, int march_steps, void* workspace, int64_t* offsets,
                         void* stream);
int nerf_occ_march_write(const float* rays, int64_t B, const float* jitter, float jitter_const, const uint32_t* bits, int log2_res,
                         float pos_scale, float pos_offset, float step_world, int march_steps, void* workspace, int64_t* offsets,
                         float* rows_out, float* z_out, void* stream);
/* Merge with a choice of density activation: NERF_OCC_RELU is nerf_occ_merge exactly; NERF_OCC_EXP (the march mode, whose field
 * density is trunc_exp(raw)) merges density = max(density * decay, exp(raw[i, 3])), a NaN raw counting as 0.               */
#define NERF_OCC_RELU 0
#define NERF_OCC_EXP 1
int nerf_occ_merge_ex(float* density, const float* raw, int64_t count, float decay, int activation, void* stream);

/* ---------------------------------------------------------------- packed compositing (no reference counterpart)
 * The reference's raw2outputs arithmetic (rendering/render.py:60-92) over the packed samples of the march, ray b owning raw /
 * z [offsets[b], offsets[b + 1]) (0 to 1024 samples; 16-byte aligned raw [K, 4]), with two differences: sigma_k =
 * trunc_exp(raw_k[3]) (forward exp(x), backward exp(min(x, 15))), and every interval is step_world long (no 1e10 on the last):
 *   x_k = sigma_k step_world, alpha_k = 1 - exp(-x_k), T_k = exp(-sum_{i<k} x_i), w_k = alpha_k T_k,
 *   rgb = sum w c (+ (1 - acc) with a white background), acc = sum w, depth = sum w z.
 * A ray without samples gets the background, acc = depth = 0.  sigma = +inf gives finite outputs and gradients; a NaN in a
 * ray's raw makes that ray's outputs NaN and no other's.  Offsets outside [0, K], decreasing, or a segment above 4096 samples
 * give NaN outputs for that ray and no access.  The training form is nerf_composite_mse_backward's: loss_out (one float the
 * caller zeroes, float atomics) += mean over B rays x 3 channels of (rgb - target)^2, upstream gradient grad_scale * 2 (rgb -
 * target) / (3 B); rgb (may be NULL) and d_raw [K, 4] written, d_raw[k, 3] through the trunc_exp backward.                   */
int nerf_composite_packed_forward(const float* raw, const float* z, const int64_t* offsets, int64_t B, int64_t K, float step_world,
                                  int white_bkgd, float* rgb, float* acc, float* depth, void* stream);
int nerf_composite_packed_mse_backward(const float* raw, const int64_t* offsets, int64_t B, int64_t K, float step_world,
                                       int white_bkgd, const float* target, float grad_scale, float* loss_out, float* rgb,
                                       float* d_raw, void* stream);

/* ---------------------------------------------------------------- distortion regulariser (no reference counterpart)
 * The distortion loss of mip-NeRF 360 (Barron et al. 2022, eq. 15) on the packed samples of the march: it penalises ray weight
 * that is spread out or split into separate clumps.  Additive: NERF_ABI_VERSION stays 3.  For ray b with samples k in
 * [offsets[b], offsets[b + 1]) in depth order, weights w_k exactly as in "packed compositing" above, S = march_steps:
 *   u_k   = (z_k - z_first) |d_b| / (S step_world): the position along the ray in units of the scene box's diagonal (S step_world =
 *           sqrt(3) 2 bound), relative to the ray's first sample, so u in [0, 1] whatever near / far and the length of d are.
 *           |d_b| is the march's norm, float(sqrt_double((d0 d0 + d1 d1) + d2 d2)) of rays[b, 3..5].
 *   delta = 1 / S: the width of an interval (every march interval is step_world long).
 *   L_b   = sum_i sum_j w_i w_j |u_i - u_j| + (delta / 3) sum_i w_i^2            (0 for a ray without samples)
 *   dL_b/dw_k = 2 sum_j w_j |u_k - u_j| + (2 delta / 3) w_k
 * The objective of a training step is MSE + dist_weight * mean over the B rays of L_b; rays without samples count with 0.
 * Because the samples are sorted the double sum is two prefix sums.  With Wl_k = sum_{j<k} w_j, Ul_k = sum_{j<k} w_j u_j and the
 * ray's totals W, U, in float32, one rounding per operation, in this order:
 *   us = |d_b| / ((float)S * step_world), u_k = (z_k - z_first) * us
 *   Wl_k, Ul_k: the sums over the 64-sample chunks before k's, added chunk total by chunk total in depth order, plus the
 *           exclusive wave scan of w (of w * u) inside the chunk; W, U: the same chain after the last chunk
 *   L_b   = 2 * sum_k w_k * (u_k * Wl_k - Ul_k) + c1 * sum_k w_k * w_k,  c1 = (1 / (float)S) / 3     (both sums: per lane over
 *           the chunks, then a wave sum; every term of the first is >= 0 up to rounding)
 *   inter_k = u_k * ((2 * Wl_k + w_k) - W) - ((2 * Ul_k + w_k * u_k) - U)        (= sum_j w_j |u_k - u_j|)
 *   G_k  += coef * (2 * inter_k + (2 * c1) * w_k),  coef = grad_scale * dist_weight * (1 / (float)B)
 * G_k is the per-sample adjoint of w_k in the training form of packed compositing; from there the term reaches d_raw[k, 3]
 * through the same transmittance chain and trunc_exp backward.  d_raw[k, 0..2] do not see it.  Wave scans make this a
 * tolerance-level contract against tests/_distortion_ref.py (as packed compositing is); run to run d_raw and dist are
 * bit-reproducible (loss_out / dist_out are sums of float atomics).
 * Edge cases: bad offsets (as above) -> the ray's outputs and dist NaN, no access; a NaN in a ray's raw or z -> that ray's
 * d_raw and dist NaN and no other ray's; sigma = +inf -> finite dist and gradients; |d_b| zero or not finite -> dist = 0 and no
 * extra gradient for that ray (the march gives such rays no samples).  rays: float32 [B, 11] (d in columns 3..5).
 *   nerf_composite_packed_distortion          nerf_composite_packed_forward plus dist [B] = L_b (forward only; acc, depth may
 *                                             be NULL).
 *   nerf_composite_packed_mse_dist_backward   nerf_composite_packed_mse_backward plus the regulariser: loss_out keeps its meaning
 *                                             (MSE only); dist_out (one float the caller zeroes; may be NULL) += mean_b L_b,
 *                                             unweighted.  dist_weight: finite, >= 0.
 * NERF_E_SHAPE for march_steps outside [1, NERF_MARCH_MAX_STEPS], step_world <= 0, a negative or non-finite dist_weight,
 * unaligned raw / d_raw; NERF_E_NULL for NULL pointers; B = 0 returns NERF_OK.  All checked before any device work.        */
int nerf_composite_packed_distortion(const float* raw, const float* z, const int64_t* offsets, const float* rays, int64_t B,
                                     int64_t K, float step_world, int march_steps, int white_bkgd, float* rgb, float* acc,
                                     float* depth, float* dist, void* stream);
int nerf_composite_packed_mse_dist_backward(const float* raw, const float* z, const int64_t* offsets, const float* rays, int64_t B,
                                            int64_t K, float step_world, int march_steps, int white_bkgd, const float* target,
                                            float grad_scale, float dist_weight, float* loss_out, float* dist_out, float* rgb,
                                            float* d_raw, void* stream);

/* ---------------------------------------------------------------- background colour (no reference counterpart)
 * Packed compositing over a background colour other than white or none, and its training form against straight (un-premultiplied)
 * RGBA targets: Instant-NGP trains on the RGBA image over a random colour per ray, put behind the target and behind the rendered
 * ray alike, so that only acc = alpha matches the target under every colour.  Additive: NERF_ABI_VERSION stays 3.
 *   bg, bg_stride   device float32; colour of ray b = bg[b * bg_stride + 0..2].  bg_stride 0: one colour (3 floats) for all rays,
 *                   3: bg [B, 3].  Any other stride is NERF_E_SHAPE.  The training entries take bg [B, 3] (stride 3).
 * Everything up to the ray sums (sum w c per channel, acc, depth, the distortion loss) is "packed compositing" / "distortion
 * regulariser" above: the same operations in the same order, the same bits.  Then, in float32, one rounding per operation:
 *   forward    rgb_c = sum_c + (1.0f - acc) * bg_c                                                      (lane 0 of the ray's wave)
 *   training   a = target_rgba[b, 3];  t_c = target_rgba[b, c] * a + bg_c * (1.0f - a)        (formed in the kernel: no composited
 *              rgb_c as in the forward;  e_c = rgb_c - t_c;  loss_out += mean of e_c^2         target goes through memory)
 *              g_c  = grad_scale * 2 * e_c * (1 / (float)(3 B))
 *              gacc = 0.0f - ((g_r * bg_r + g_g * bg_g) + g_b * bg_b)                          (the one changed adjoint term)
 *              G_k  = g_r r_k + g_g g_k + g_b b_k + gacc, and from there the suffix sums, the trunc_exp backward and the
 *              distortion term added to G_k exactly as above.
 *   finish     nerf_ert_finish with rgb_c = state_c + (1.0f - acc) * bg_c.
 * Three identities follow (multiplying by 1.0f is exact; the library is built without FMA contraction):
 *   bg = (1, 1, 1)  the forward entries give the bits of white_bkgd = 1; the training entries those of the white_bkgd = 1
 *                   entries fed the same t.
 *   a = 1           t_c = target_rgba[b, c] exactly (finite bg).
 *   bg = (0, 0, 0)  with a finite acc the outputs equal those of white_bkgd = 0, except that a zero may change its sign.
 * Edge cases as above (bad offsets -> that ray NaN, no access; sigma = +inf finite; B = 0 and K = 0 succeed; acc, depth, loss_out,
 * dist_out, rgb of the training forms, samples may be NULL), and a NaN in a ray's bg or target makes that ray's outputs and
 * d_raw NaN and no other ray's (loss_out, one sum over the batch, is NaN too).  No atomics beyond loss_out / dist_out.
 * target_rgba must be 16-byte aligned like raw / d_raw (NERF_E_SHAPE).  All checks run before any device work.               */
int nerf_composite_packed_forward_bg(const float* raw, const float* z, const int64_t* offsets, int64_t B, int64_t K, float step_world,
                                     const float* bg, int bg_stride, float* rgb, float* acc, float* depth, void* stream);
int nerf_composite_packed_distortion_bg(const float* raw, const float* z, const int64_t* offsets, const float* rays, int64_t B,
                                        int64_t K, float step_world, int march_steps, const float* bg, int bg_stride, float* rgb,
                                        float* acc, float* depth, float* dist, void* stream);
int nerf_composite_packed_mse_backward_bg(const float* raw, const int64_t* offsets, int64_t B, int64_t K, float step_world,
                                          const float* target_rgba, const float* bg, float grad_scale, float* loss_out, float* rgb,
                                          float* d_raw, void* stream);
int nerf_composite_packed_mse_dist_backward_bg(const float* raw, const float* z, const int64_t* offsets, const float* rays, int64_t B,
                                               int64_t K, float step_world, int march_steps, const float* target_rgba,
                                               const float* bg, float grad_scale, float dist_weight, float* loss_out,
                                               float* dist_out, float* rgb, float* d_raw, void* stream);

/* ---------------------------------------------------------------- early ray termination (no reference counterpart)
 * The round renderer of the march (inference only): a ray stops once its transmittance falls below min_transmittance = eps
 * (0 <= eps < 1), and the steps behind that point are neither marched nor queried.  Additive: NERF_ABI_VERSION stays 3.
 *   samples   a ray visits exactly the candidates of nerf_occ_march_count / _write ("ray march" above): the same depths (z_k uses
 *             the absolute candidate index k), the same keep decisions, the same march_steps cap, in depth order.  A round resumes
 *             at the ray's saved k and kept count.  With eps = 0 the (ray, depth) samples are those of the one-shot march, bit for bit.
 *   fold      serial over a ray's samples in depth order, float32, one rounding per operation, in this order:
 *               T = expf(-carry); if T < eps the ray terminates: this sample and every later one are skipped (NaN T does not);
 *               x = expf(raw[3]) * step_world, alpha = 1 - expf(-x), w = alpha * T;
 *               r += w raw[0], g += w raw[1], b += w raw[2], acc += w, depth += w z, carry += x, samples += 1.
 *             At the end rgb += (1 - acc) with a white background.  A ray without samples gets the background, acc = depth = 0.
 *             Because the fold is serial per ray, a ray's outputs depend on that ray and the field only: round sizes, chunking and
 *             ray order change no bit.  Against the one-shot renderer (packed compositing above): |d rgb| <= T_stop max|c - bg|
 *             < eps per channel, 0 <= acc_full - acc_eps < eps (up to float rounding), samples_eps <= samples_full.
 *             sigma = +inf gives finite outputs (and terminates the ray when eps > 0); a NaN raw makes only its own ray NaN.
 * State (caller memory, reused between calls): istate int32 [B, 4] = (next candidate k, kept count, samples folded, flags),
 * fstate float [B, 6] = (carry, r, g, b, acc, depth), a list of live ray ids (int32, ascending, distinct), B < 2^31.  A call:
 *   nerf_ert_init                  zero state, live = 0 .. B - 1, A = B.
 *   per round, with m >= 1 slots per live ray:
 *     nerf_ert_march_count         per live entry up to m further kept samples (none for a terminated ray); totals int64 [2] =
 *                                  (K samples of the round, A' rays still live: those that took m and have candidates left).
 *     (one read of totals to the host; K = 0 ends the call)
 *     nerf_ert_march_write         same arguments and workspace: offsets int64 [A + 1] (entry i owns [offsets[i], offsets[i + 1]),
 *                                  offsets[A] = K), rows_out [K, 11], z_out [K] (the layout of the march above), live_out [A']
 *                                  (must not be live), and the resume point in istate.  No atomics: bit-reproducible.
 *     query of the K rows           (nerf_ngp_query_fused_h, B = K, n = 1)
 *     nerf_ert_fold                the fold over entry i's segment for ray live[i], raw [K, 4] (16-byte aligned), z [K].  A ray
 *                                  whose next sample would terminate is flagged now (same outputs, no further march).
 *   nerf_ert_finish                rgb [B, 3], and (each may be NULL) acc [B], depth [B], samples int32 [B].
 * workspace: nerf_ert_march_workspace_bytes(B) bytes, kept from the count to the write of a round.  A live id outside [0, B)
 * takes no sample and is not folded; offsets outside [0, K] or decreasing make that ray's outputs NaN.                      */
#define NERF_ERT_TERMINATED 1
int64_t nerf_ert_march_workspace_bytes(int64_t B);
int nerf_ert_init(int64_t B, int32_t* istate, float* fstate, int32_t* live, void* stream);
int nerf_ert_march_count(const float* rays, int64_t B, const float* jitter, float jitter_const, const uint32_t* bits, int log2_res,
                         float pos_scale, float pos_offset, float step_world, int march_steps, const int32_t* live, int64_t A,
                         const int32_t* istate, int max_new, void* workspace, int64_t* totals, void* stream);
int nerf_ert_march_write(const float* rays, int64_t B, const float* jitter, float jitter_const, const uint32_t* bits, int log2_res,
                         float pos_scale, float pos_offset, float step_world, int march_steps, const int32_t* live, int64_t A,
                         int32_t* istate, int max_new, void* workspace, int64_t* offsets, int32_t* live_out, float* rows_out,
                         float* z_out, void* stream);
int nerf_ert_fold(const float* raw, const float* z, const int64_t* offsets, const int32_t* live, int64_t A, int64_t B, int64_t K,
                  float step_world, float min_transmittance, int32_t* istate, float* fstate, void* stream);
int nerf_ert_finish(const int32_t* istate, const float* fstate, int64_t B, int white_bkgd, float* rgb, float* acc, float* depth,
                    int32_t* samples, void* stream);
int nerf_ert_finish_bg(const int32_t* istate, const float* fstate, int64_t B, const float* bg, int bg_stride, float* rgb, float* acc,
                       float* depth, int32_t* samples, void* stream);    /* "background colour" above */

/* ---------------------------------------------------------------- mesh extraction (no reference counterpart)
 * Marching cubes over a density volume sampled from a trained field (Instant-NGP's mesh export).  Additive: NERF_ABI_VERSION
 * stays 3.  Float32, one rounding per operation, in this order (tests/_mesh_ref.py reproduces every output):
 *   lattice   box lo[3] < hi[3] (host floats, finite), resolution R (2 <= R <= NERF_MESH_MAX_RES), h_a = (hi_a - lo_a) / R
 *             computed on the host.  Point (i, j, k), 0 <= i, j, k < R, has linear index i + R (j + R k) and position
 *             p_a = lo_a + ((float)i_a + 0.5f) * h_a: cell centres, strictly inside the box.  vol: float32 [R, R, R] = vol[k, j, i].
 *   density   (the caller; engine/mesh.py) sigma = act(raw[..., 3]) of the field's fused query on the rows of nerf_mesh_points
 *             (o = p, the rest 0, z = 0), act = exp for the march mode's field, relu otherwise, NaN counting as 0: exactly
 *             nerf_occ_merge_ex(slice, raw, n, decay = 0, act) on a zeroed slice.
 *   inside    v > iso (iso finite): NaN and v == iso are outside.
 *   cells     cell (i, j, k), all < R - 1, has corner c in [0, 8) at (i + (c & 1), j + ((c >> 1) & 1), k + (c >> 2)); its case is
 *             sum inside(c) << c, its triangles the case's row of csrc/mc_table.h (generated by csrc/gen_mc_table.py from the face
 *             rule stated there: neighbouring cells agree on every shared face, so the mesh is closed and consistently oriented
 *             wherever the surface stays inside the box).  Winding: (b - a) x (c - a) points from inside to outside.
 *   vertices  the edge from point q to q + e_a is owned by q; a crossing edge (one end inside) carries exactly one vertex, so the
 *             mesh is welded by construction.  Order: by owner linear index, then axis x, y, z.  Position: p(q), and along a
 *             t = (iso - v_q) / (v_{q+e_a} - v_q) (correctly rounded), t = 0.5 if t is NaN, else t clamped to [0, 1];
 *             x_a = p_a(q) + t * h_a.  V <= 3 R^3 < 2^31: vertex ids are int32.
 *   normals   g = the volume's gradient at the two ends, (v[+1] - v[-1]) / (2 h_a), one-sided (v[1] - v[0]) / h_a at the border,
 *             interpolated as g0 + t (g1 - g0); |g| = sqrt((gx gx + gy gy) + gz gz); n = -(g / |g|), or 0 where |g| is 0 or not
 *             finite (divisions and the square root correctly rounded).
 *   faces     int32 [F, 3] vertex ids, by cell linear index, then table order.
 * Calls: nerf_mesh_count writes totals int64 [2] = (V, F) (the caller reads them once and sizes the outputs); then, with the
 * same volume, iso and workspace, nerf_mesh_write_vertices (verts [V, 3], normals [V, 3], and when color_rows != NULL the colour
 * query rows [V, 11] = [x, -n, near = far = 0, viewdirs = -n]) and nerf_mesh_write_faces (faces [F, 3]).  V = 0 exactly when
 * F = 0; then the write calls launch nothing.  Count -> block scan -> write, no atomics: bit-reproducible.
 * workspace: nerf_mesh_workspace_bytes(R) bytes, kept from the count to the faces (the per-point vertex bases live there).
 * Argument errors (R, box, non-finite iso, V / F out of range, NULL) return before any launch.                              */
#define NERF_MESH_MAX_RES 512
int64_t nerf_mesh_workspace_bytes(int res);
int nerf_mesh_points(int res, const float* lo_host, const float* hi_host, int64_t p0, int64_t count, float* rays_out, float* z_out,
                     void* stream);
int nerf_mesh_count(const float* vol, int res, float iso, void* workspace, int64_t* totals, void* stream);
int nerf_mesh_write_vertices(const float* vol, int res, float iso, const float* lo_host, const float* hi_host, void* workspace,
                             int64_t V, float* verts, float* normals, float* color_rows, void* stream);
int nerf_mesh_write_faces(const float* vol, int res, float iso, void* workspace, int64_t F, int32_t* faces, void* stream);

/* ---------------------------------------------------------------- connected components (no reference counterpart)
 * The 6-connected components of {v > iso} of a mesh-extraction volume, and the filter that drops the small ones (the floaters of
 * a trained field) before marching cubes.  Additive: NERF_ABI_VERSION stays 3.  vol: contiguous float32 [R, R, R] with the
 * conventions of "mesh extraction": linear index p = i + R (j + R k), inside iff v > iso (NaN and v == iso are outside),
 * 2 <= R <= NERF_MESH_MAX_RES, iso finite.  tests/_ccl_ref.py reproduces every output bit for bit.
 *   labels    int32 [R^3]: -1 at an outside voxel; at an inside voxel the smallest linear index of its component.  Neighbours
 *             are +-1 along one axis inside the lattice (no wrap from i = R - 1 to the next row's i = 0).  The rule defines the
 *             output uniquely: any algorithm and any scheduling give the same bits.
 *   sizes     int32 [R^3]: the component's voxel count at its root (labels[p] == p), 0 elsewhere (integer atomics: exact).
 *   stats     int64 [3]: the number of components, the number of inside voxels, and the label of the largest component (the
 *             most voxels, ties to the smaller label) or -1 when there is none.
 *   filter    out[p] = dropped(p) ? iso : vol[p], float32 [R^3]; every kept or outside voxel (NaN included) is copied bit for
 *             bit.  An inside voxel is dropped when its component has fewer than min_voxels voxels (min_voxels >= 0; 0 and 1
 *             drop nothing) or, with largest_only != 0, when its component is not the largest one.  If the largest component
 *             has fewer than min_voxels voxels nothing survives.  out may alias vol.  A dropped voxel is outside (iso > iso is
 *             false) and leaves the central differences of the normals finite.
 *   sub-mesh  No lattice edge joins a dropped voxel to a kept inside voxel (they would share a component).  Every crossing edge
 *             of the filtered volume is therefore a crossing edge of the original with both end values unchanged: the vertices
 *             of marching cubes on the filtered volume are, bit for bit and in the same order, the subsequence of the original's
 *             vertices whose inside end is kept.  The case table's face rule keeps the two inside corners of a face diagonal
 *             apart, so the mesh separates exactly the pieces 6-connectivity separates.  Normals are those of the filtered
 *             volume: next to a dropped voxel they may differ from the original mesh's.
 * Calls: nerf_ccl_label (three launches: runs along x inside a workgroup, unions across y / z with atomicMin on the parent array
 * in the workspace -- the smaller root wins, so a root is its component's minimum --, flatten), nerf_ccl_sizes (four launches),
 * nerf_ccl_filter (one).  The number of launches depends on R alone and nothing is read on the host; the filter reads sizes
 * and stats from device memory.  workspace: nerf_ccl_workspace_bytes(R) bytes of unspecified content, used by nerf_ccl_label
 * only.  Argument errors (R, non-finite iso, min_voxels < 0, NULL) return before any launch.                                  */
int64_t nerf_ccl_workspace_bytes(int res);
int nerf_ccl_label(const float* vol, int res, float iso, void* workspace, int32_t* labels, void* stream);
int nerf_ccl_sizes(const int32_t* labels, int res, int32_t* sizes, int64_t* stats, void* stream);
int nerf_ccl_filter(const float* vol, const int32_t* labels, const int32_t* sizes, const int64_t* stats, int res, float iso,
                    int64_t min_voxels, int largest_only, float* out, void* stream);

/* ---------------------------------------------------------------- morphological opening (no reference counterpart)
 * An erosion ahead of the connected-component filter, to cut the thin bridges that tie a floater to the surface, and the
 * geodesic reconstruction that gives what the filter kept its skin back.  Additive: NERF_ABI_VERSION stays 3.  Volumes as in
 * "connected components": contiguous float32 [R, R, R], p = i + R (j + R k), inside set M = {v > iso} (NaN and v == iso are
 * outside), 2 <= R <= NERF_MESH_MAX_RES, iso finite; neighbours are +-1 along one axis inside the lattice (i = R - 1 and the next
 * row's i = 0 are not neighbours).  radius r: 1 <= r <= NERF_MORPH_MAX_RADIUS; the structuring element is the 6-neighbour (L1)
 * ball of radius r = r iterations of the 6-neighbour step.  tests/_morph_ref.py reproduces every output bit for bit.
 *   erode        E_0 = M; E_{n+1}[p] = E_n[p] and all six neighbours are in E_n, a neighbour beyond the lattice counting as
 *                outside (the box faces erode too); E = E_r.  core[p] = (p in M \ E) ? iso : vol[p]; every other voxel (NaN
 *                included) is copied bit for bit.  core is again a volume of these conventions: nerf_ccl_* run on it unchanged.
 *                core may alias vol.  stats2 = (|M|, |E|).
 *   reconstruct  seeds K = {kept > iso} within M (a seed outside M is ignored); D_0 = K; D_{n+1} = (D_n united with the six
 *                neighbours of D_n) within M: geodesic dilation, exactly r steps, not to convergence.  out[p] = (p in M \ D_r) ? iso : vol[p];
 *                everything else is copied bit for bit.  out may alias vol or kept.  stats2 = (|K|, |D_r|).
 *   stats2       int64 [2], exact integer reductions (integer atomics, in any order).
 *   pipeline     (engine/mesh.py open_components) core = erode(vol); kept = nerf_ccl_filter(core) or core itself; out =
 *                reconstruct(vol, kept).  min_voxels of the filter then counts CORE voxels.
 * Properties (tests/test_morph_host.py checks each on the reference):
 *   - E is the direct definition: p is in E exactly when every lattice point within L1 distance r of p is in M and none of
 *     those points lies beyond the lattice.
 *   - E (+) ball_r is a subset of D_r, D_r a subset of M (with K = E, or K any union of components of E): the reconstruction
 *     gives back at least the classical opening, and keeps thin detail within r steps of a kept core.  It never crosses a gap:
 *     two arms of M closer than r in L1 but farther apart inside M do not seed each other.
 *   - With K = E, erode(out) has the core E again: the operation is idempotent.
 *   - Sub-mesh, weaker than the filter's: a crossing edge of `out` whose outside end was outside in vol carries the original
 *     mesh's vertex bit for bit, and these keep their order; an edge whose outside end is a dropped voxel (value iso exactly)
 *     carries a new cut vertex on the dropped voxel (t = 1 counted from the kept end).
 *   - A field thinner than 2 r + 1 voxels everywhere has an empty core: everything is dropped and the mesh is empty.  That is
 *     the definition, not an error.
 * Calls: pack (one wave's ballot of v > iso over 64 consecutive x is a mask word; rows are padded to whole 64-bit words, the dead
 * bits 0), r steps on the bit masks (one lane per word; y / z neighbours are whole words, x neighbours a shift with a carry bit
 * from the adjacent word of the same row), apply (one lane per voxel): r + 2 launches per call, decided by (R, r) alone; nothing
 * is read on the host; every output bit has one writer.  workspace: nerf_morph_workspace_bytes(R) bytes of unspecified content
 * (three masks), not kept between calls.  Argument errors (R, non-finite iso, radius, NULL) return before any launch.          */
#define NERF_MORPH_MAX_RADIUS 16
int64_t nerf_morph_workspace_bytes(int res);
int nerf_morph_erode(const float* vol, int res, float iso, int radius, void* workspace, float* core, int64_t* stats2, void* stream);
int nerf_morph_reconstruct(const float* vol, const float* kept, int res, float iso, int radius, void* workspace, float* out,
                           int64_t* stats2, void* stream);

/* ---------------------------------------------------------------- pinhole camera (no reference counterpart)
 * The one camera of "TSDF fusion", "mesh rendering", "view-projected texture" and "texture mip pyramid": they must agree bit for
 * bit (the bake tests a texel against the depth map the rasteriser drew, fusion integrates that depth, the level of detail calls the
 * rasteriser's setup).  csrc/camera.h states it in code; tests/_camera_ref.py is its numpy reference.  IEEE float32, one rounding
 * per operation (no contraction), in exactly the order and grouping written here; a / b correctly rounded.
 *   view      nerf_tsdf_view (below), 16 finite floats on the host: c2w [3, 4] row-major (r_ab = c2w[4 a + b], t_a = c2w[4 a + 3];
 *             camera directions [(col - cx) / fx, -(row - cy) / fy, -1] at integer pixel centres, as nerf_ray_gen), then fx, fy, cx,
 *             cy (the K doubles cast once on the host).  A non-finite number is NERF_E_SHAPE.
 *   point     a world point p: q_a = p_a - t_a; x_c = (r00 q0 + r10 q1) + r20 q2, y_c with column 1, z_w with column 2;
 *             zc = 0.0f - z_w, the distance along the optical axis (what depth / acc of a renderer's aux maps means).
 *   pixel     u = fx (x_c / zc) + cx; v = cy - fy (y_c / zc).  Pixel (px, py), py the image row, has its centre at (u, v) =
 *             (px, py): the ray nerf_ray_gen shoots.  Each user says whether it tests zc before or after the division.
 *   nearest   the pixel of an [H, W] map nearest to (u, v): fu = floorf(u + 0.5f), fv = floorf(v + 0.5f); outside unless
 *             0 <= fu < W and 0 <= fv < H, compared as floats (a non-finite or huge u, v fails here, before any conversion);
 *             inside, i = (int)fu, j = (int)fv and the map is read at j W + i.
 *   batch     an entry that takes n views takes n structs on the host and hands at most 16 to a launch by value.                 */

/* ---------------------------------------------------------------- TSDF fusion (no reference counterpart)
 * Fuses rendered depth / opacity maps of posed pinhole cameras into a truncated signed distance volume on the lattice of "mesh
 * extraction" (KinectFusion; nerfstudio's TSDF export), whose zero level set is the other mesh of a trained field: a voxel is
 * inside only if the cameras agree a surface lies in front of it.  Additive: NERF_ABI_VERSION stays 3.  Lattice as above: box
 * lo[3] < hi[3] (host floats, finite), 2 <= R <= NERF_MESH_MAX_RES, h_a = (hi_a - lo_a) / R on the host, point (i, j, k) has linear
 * index p = i + R (j + R k) and position p_a = lo_a + ((float)i_a + 0.5f) * h_a.  Float32, one rounding per operation, in this
 * order (divisions correctly rounded; tests/_tsdf_ref.py reproduces every output bit for bit):
 *   state     D float32 [R^3], the running mean of the truncated distance in units of the truncation tau; Wt float32 [R^3], the
 *             number of observations; flags uint8 [R^3], bit 0 = occluded in at least one view.  nerf_tsdf_reset zeroes all three.
 *   view      a nerf_tsdf_view of "pinhole camera"; maps depth [H W] and acc [H W] as a renderer's aux outputs: depth = sum w z with z the
 *             parameter of o + z d for the unnormalised d whose camera z is -1, so depth / acc is distance along the optical axis.
 *   per voxel and view, with tau > 0, 0 < acc_min <= 1, far > 0, carve in {0, 1}:
 *             zc of the camera's `point`; !(zc > 0): no observation (NaN included).  (u, v) of its `pixel` and (i, j) of its
 *             `nearest`; outside the map: no observation.  a = acc[j W + i], s = depth[j W + i]; a or s NaN: no observation.  a < acc_min: with carve and zc <= far the observation d = 1.0f (the ray hit nothing: empty all along
 *             it), else none.  Otherwise e = s / a - zc; e < -tau: flags |= 1, no observation; e NaN: none; else
 *             d = fminf(1.0f, e / tau).  On an observation: Wn = Wt + 1.0f; D = (D Wt + d) / Wn; Wt = Wn.
 *   batch     nerf_tsdf_integrate folds n <= NERF_TSDF_MAX_VIEWS views (views_host: n structs on the host, passed by value as
 *             kernel arguments; depth, acc: device [n, H W]) in order in ONE launch: one lane per voxel loads its state once, keeps
 *             it in registers over the views and stores it once.  Bit-identical to n calls of one view in the same order.  n = 0
 *             launches nothing.  No atomics, nothing read on the host, one writer per voxel: bit-reproducible.
 *   finish    nerf_tsdf_volume: vol[p] = 0.0f - D[p] where Wt[p] >= (float)min_views (min_views >= 1); else +1.0f where flags bit 0
 *             is set (seen only from behind a surface: inside -- without this every surface gets an inner twin at depth tau); else
 *             -1.0f (never seen: outside).  vol is a volume of "mesh extraction" at iso = 0 (inside = D < 0): nerf_mesh_*, nerf_ccl_*
 *             and nerf_morph_* run on it unchanged.
 * Argument errors (R, box, n outside [0, 16], H, W outside [1, 2^24], non-positive or non-finite trunc / far, acc_min outside
 * (0, 1], carve not 0 / 1, a non-finite camera number, min_views < 1, NULL) return before any launch.                          */
#define NERF_TSDF_MAX_VIEWS 16
typedef struct nerf_tsdf_view {
  float c2w[12];
  float fx, fy, cx, cy;
} nerf_tsdf_view;
int nerf_tsdf_reset(float* D, float* Wt, uint8_t* flags, int res, void* stream);
int nerf_tsdf_integrate(float* D, float* Wt, uint8_t* flags, int res, const float* lo_host, const float* hi_host,
                        const nerf_tsdf_view* views_host, int n, int H, int W, const float* depth, const float* acc, float trunc,
                        float acc_min, float far, int carve, void* stream);
int nerf_tsdf_volume(const float* D, const float* Wt, const uint8_t* flags, int res, int min_views, float* vol_out, void* stream);

/* ---------------------------------------------------------------- mesh simplification (no reference counterpart)
 * Vertex clustering (Rossignac-Borrel) with quadric placement (Lindstrom's out-of-core simplification): the decimation step
 * behind marching cubes.  Additive: NERF_ABI_VERSION stays 3.  All arithmetic is IEEE double, one rounding per operation, in
 * exactly the order and grouping written here, unless it says int64; tests/_simplify_ref.py reproduces every output bit for bit.
 *   input     verts [V, 3] float32, faces [F, 3] int32, normals [V, 3] float32, colors [V, 3] float32 or NULL; box lo[3] < hi[3]
 *             (host floats, finite); grid G, 2 <= G <= NERF_MESH_MAX_RES; 0 <= V, F <= 2^24; min(V, G^3) <= 2^21 (the bound on
 *             the cluster count that is known without a host read: cluster ids must fit the 21-bit fields of the face key).
 *             Outside these ranges: NERF_E_SHAPE; NULL: NERF_E_NULL.  V = 0 or F = 0: the empty mesh, nothing is launched.
 *   cells     ext_a = (double)hi_a - (double)lo_a; c_a = ext_a / G; inv_a = G / ext_a; t_a = ((double)v_a - lo_a) * inv_a;
 *             q_a = min(max(floor(t_a), 0), G - 1); key = (q_z G + q_y) G + q_x.  A vertex is invalid when some t_a is not
 *             finite (a non-finite coordinate always is): it joins no cluster, and every face that uses it is dropped.  A face
 *             with an index outside [0, V) is dropped too, and nothing is read through that index.
 *   clusters  the occupied cells, numbered in ascending key order; K of them.
 *   sums      exact int64, independent of the arrival order.  fix(x, L, s) = (int64)rint(min(max(x, -L), L) * s), 0 for a NaN x
 *             (rint: to nearest, ties to even).  Local coordinates of a point with lattice coordinates t in the cluster of cell
 *             q: u_a = t_a - (q_a + 0.5).  Per cluster, over its vertices: n = the count; S_a = sum fix(u_a, 64, 2^32) (the clamp
 *             only touches vertices 64 cells outside the box); N_a = sum fix(normal_a, 256, 2^30), a non-finite component
 *             counting as 0; with colours C_a = sum rint(min(max(color_a, 0), 1) * 2^30), NaN counting as 0.
 *   quadrics  for every face with three valid corners (also one that turns out degenerate or annihilated), once for every
 *             distinct cluster among its corners, in that cluster's local coordinates u0, u1, u2 of the three corners:
 *             e1 = u1 - u0, e2 = u2 - u0, n = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x),
 *             d = -((nx u0x + ny u0y) + nz u0z); the nine sums Q = (Axx, Axy, Axz, Ayy, Ayz, Azz, bx, by, bz) receive
 *             fix(x, 64, 2^32) for x = nx nx, nx ny, nx nz, ny ny, ny nz, nz nz, nx d, ny d, nz d: area^2-weighted.  The clamp
 *             and the limit on F keep every sum inside int64.
 *   placement ubar_a = S_a / 2^32 / n.  A.. and b. below are the sums / 2^32.  With NERF_SIMPLIFY_MEAN, or when
 *             tr = (Axx + Ayy) + Azz <= 0: x = ubar.  Otherwise mu = (tr / 3) * 2^-10, and (A + mu I) x = mu ubar - b by Cramer's
 *             rule: a00 = Axx + mu, a01 = Axy, a02 = Axz, a11 = Ayy + mu, a12 = Ayz, a22 = Azz + mu; r_a = mu ubar_a - b_a;
 *             c00 = a11 a22 - a12 a12, c01 = a02 a12 - a01 a22, c02 = a01 a12 - a02 a11, c11 = a00 a22 - a02 a02,
 *             c12 = a01 a02 - a00 a12, c22 = a00 a11 - a01 a01; det = (a00 c00 + a01 c01) + a02 c02;
 *             x0 = ((c00 r0 + c01 r1) + c02 r2) / det, x1 = ((c01 r0 + c11 r1) + c12 r2) / det,
 *             x2 = ((c02 r0 + c12 r1) + c22 r2) / det.  x is taken when all three are finite and |x_a| <= 0.5, else x = ubar.
 *             The mu term pulls towards the mean: it decides the position along a flat face or a straight edge, where A alone is
 *             singular.  Vertex: (float)(lo_a + ((q_a + 0.5) + x_a) * c_a).
 *   normals   s_a = N_a / 2^30, len = sqrt((sx sx + sy sy) + sz sz); (float)(s_a / len) when len > 0, else 0.
 *   colours   (float)(C_a / 2^30 / n).
 *   faces     every corner becomes its cluster; a face with two equal corners is dropped.  Among the remaining faces on one
 *             vertex set, p with one orientation and m with the other, the first min(p, m) of each orientation in input order are
 *             dropped: opposite faces annihilate, a one-voxel-thick sheet vanishes.  Survivors keep their corner order and their
 *             input order.
 *   compact   clusters that no surviving face uses are dropped, the others keep ascending key order, faces are renumbered: no
 *             isolated vertex; if every directed edge of the input occurs as often as its reverse, so does every one of the output.
 * Calls, with the same (V, faces, F, box, G) and workspace throughout:
 *   nerf_simplify_cluster  keys, occupancy bit mask over G^3 with per-word prefix counts, ranks, the sums (64-bit integer
 *                          atomics), and per face tri_keys int64 [F]: (lo << 42) | (mid << 21) | hi of its sorted cluster triple,
 *                          INT64_MAX for a dropped face.  Its orientation stays in the workspace.
 *   (the caller)           a STABLE ascending sort of tri_keys: sorted_keys [F] and perm int64 [F], sorted_keys[i] = tri_keys[perm[i]].
 *   nerf_simplify_count    survivors inside the sorted runs in constant work per face (one scan carries the run heads and one
 *                          orientation's prefix; a run of any length costs its length), used clusters, both compactions'
 *                          counts.  totals int64 [3] = (V', F', K): the one host read.
 *   nerf_simplify_write    verts_out [V', 3], normals_out [V', 3], colors_out [V', 3] (NULL without input colours), color_rows
 *                          [V', 11] or NULL (the rows of nerf_mesh_write_vertices: [x, -n, 0, 0, -n]), faces_out [F', 3].  Nothing
 *                          is written past V_out vertices or F_out faces.
 * No float atomics, every output element has one writer: bit-reproducible, and independent of the order of the input's vertices
 * and faces up to the order of the output faces.  workspace: nerf_simplify_workspace_bytes(V, F, G) bytes (-1 for arguments out
 * of range), kept from the cluster call to the write call; its content on entry is unspecified.  All argument checks run before
 * any device work.
 * Not done: no edge-collapse decimation to a target face count, no texture atlas, no guarantee of manifoldness after clustering. */
#define NERF_SIMPLIFY_MEAN 0
#define NERF_SIMPLIFY_QUADRIC 1
int64_t nerf_simplify_workspace_bytes(int64_t V, int64_t F, int grid);
int nerf_simplify_cluster(const float* verts, const float* normals, const float* colors, int64_t V, const int32_t* faces, int64_t F,
                          const float* lo_host, const float* hi_host, int grid, void* workspace, int64_t* tri_keys, void* stream);
int nerf_simplify_count(const int64_t* sorted_keys, const int64_t* perm, int64_t V, const int32_t* faces, int64_t F, int grid,
                        void* workspace, int64_t* totals, void* stream);
int nerf_simplify_write(int64_t V, const int32_t* faces, int64_t F, const float* lo_host, const float* hi_host, int grid,
                        int placement, void* workspace, int64_t V_out, int64_t F_out, float* verts_out, float* normals_out,
                        float* colors_out, float* color_rows, int32_t* faces_out, void* stream);

/* ---------------------------------------------------------------- mesh smoothing (no reference counterpart)
 * Taubin's lambda|mu filter ("A signal processing approach to fair surface design", 1995): an umbrella-Laplacian half-step with
 * lambda > 0, then one with mu < 0; it takes the voxel-scale noise off a marching-cubes mesh without the shrinkage of plain
 * Laplacian smoothing.  The step between marching cubes and the simplifier.  Additive: NERF_ABI_VERSION stays 3.  All arithmetic
 * is IEEE double, one rounding per operation, in exactly the order and grouping written here, unless it says int64;
 * tests/_smooth_ref.py reproduces every output bit for bit.
 *   input     verts [V, 3] float32, faces [F, 3] int32; box lo[3] < hi[3] (host floats, finite); 0 <= V, F <= 2^24.
 *             ext_a = (double)hi_a - (double)lo_a, ctr_a = ((double)lo_a + (double)hi_a) * 0.5.
 *   ignored   a face with an index outside [0, V) or with two equal corners is ignored entirely: nothing is read through a bad
 *             index, and dropping such a face from the input changes no output bit.
 *   rows      every remaining face (a, b, c) adds one entry to the row of each corner, the other two corners in face order: row a
 *             receives (b, c), row b (c, a), row c (a, b).  The weight of a neighbour in the umbrella is so the number of faces
 *             on the shared edge (2 on a closed manifold, 1 along a boundary), and an entry keeps the face's orientation.
 *   sums      exact int64, independent of the arrival order.  fix(x, L, s) = (int64)rint(min(max(x, -L), L) * s), 0 for a NaN x
 *             (rint: to nearest, ties to even), as in the simplifier.
 *   half-step with factor k (a float32 argument, used as (double)k), float32 positions in, float32 positions out.  A position is
 *             finite when its three coordinates are.  For vertex a with a finite position v: over the entries of its row, for
 *             each of the entry's two neighbours whose position w is finite, S_x += fix(u_x, 4, 2^32) with
 *             u_x = ((double)w_x - ctr_x) / ext_x per axis x, and n counts the positions added.  One unit is 2^-32 of the extent;
 *             a row of 2^24 entries adds 2^25 positions of at most 2^34 units each, below 2^63; the clamp only touches
 *             neighbours 3.5 extents outside the box.  mean_x = ctr_x + (S_x / 2^32 / n) * ext_x;
 *             out_x = (float)((double)v_x + k * (mean_x - (double)v_x)).  A vertex with n = 0, or whose own position is not
 *             finite, is copied bit for bit.
 *   run       `iterations` pairs: a half-step with lambda, then one with mu.  mu = 0 is plain Laplacian smoothing: the second
 *             half-step is not launched.  0 < lambda <= 1; mu = 0 or -2 <= mu < 0; 1 <= iterations <= 1024; NaN is refused.
 *             verts_in is never written; verts_in and verts_out must not overlap.
 *   normals   for vertex a with a finite position v, over the entries (b, c) of its row whose two positions are finite:
 *             d1_x = ((double)v_b,x - (double)v_x) / ext_x, d2_x = ((double)v_c,x - (double)v_x) / ext_x, the cross product in box
 *             units c = (d1y d2z - d1z d2y, d1z d2x - d1x d2z, d1x d2y - d1y d2x), N_x += fix(c_x, 16, 2^34).  Back in world
 *             units (a cross product scales by the other two extents) s_x = (N_x / 2^34) * (ext_y * ext_z),
 *             s_y = (N_y / 2^34) * (ext_z * ext_x), s_z = (N_z / 2^34) * (ext_x * ext_y): the sum of the face normals
 *             (v_b - v_a) x (v_c - v_a), weighted by area.  2^24 entries of at most 16 * 2^34 units stay below 2^63; a face
 *             spanning one cell of an R = 512 lattice has c = 2^-18, 2^16 units; the clamp only touches faces with an edge
 *             longer than 2.8 extents.  len = sqrt((sx sx + sy sy) + sz sz); (float)(s_x / len) when len > 0, else 0 (an
 *             unreferenced or non-finite vertex).  color_rows [V, 11] or NULL: the rows [x, -n, 0, 0, -n] of
 *             nerf_mesh_write_vertices.
 * Calls, with the same V and workspace throughout:
 *   nerf_smooth_build      entries per vertex (integer atomics), their exclusive scan, the entries through per-row cursors.  The
 *                          order inside a row depends on the arrival order; no result does.  No sort, no host read.
 *   nerf_smooth_run        2 * iterations half-steps (iterations with mu = 0), one lane per vertex, alternating between verts_out
 *                          and one workspace buffer so that the last one writes verts_out.
 *   nerf_smooth_normals    normals_out [V, 3] (and color_rows) of `verts` over the rows of the build.
 * Faces are not touched: the connectivity, orientation and closedness of the input are those of the output.  No float atomics,
 * every output element has one writer: bit-reproducible, independent of the order of the faces, equivariant under a renumbering
 * of the vertices.  workspace: nerf_smooth_workspace_bytes(V, F) bytes (-1 for arguments out of range), kept from the build on;
 * its content on entry is unspecified.  Out of range: NERF_E_SHAPE; NULL: NERF_E_NULL; all argument checks run before any device
 * work.  V = 0: nothing is launched.  F = 0: the build zeroes the row offsets with one memset and launches nothing; run and
 * normals, which are not told F, then copy V rows and write V zero normals.
 * Not done: no cotangent weights, no feature-preserving (bilateral) smoothing, no pinning of the vertices on the box faces, no
 * smoothing of the density volume before marching cubes, no change to the simplifier's arithmetic.                                */
int64_t nerf_smooth_workspace_bytes(int64_t V, int64_t F);
int nerf_smooth_build(int64_t V, const int32_t* faces, int64_t F, void* workspace, void* stream);
int nerf_smooth_run(const float* verts_in, int64_t V, const float* lo_host, const float* hi_host, int iterations, float lambda,
                    float mu, void* workspace, float* verts_out, void* stream);
int nerf_smooth_normals(const float* verts, int64_t V, const float* lo_host, const float* hi_host, void* workspace,
                        float* normals_out, float* color_rows, void* stream);

/* ---------------------------------------------------------------- edge-collapse decimation (no reference counterpart)
 * Decimation to a target face count: greedy quadric-error edge collapse (Garland-Heckbert, "Surface simplification using quadric
 * error metrics", 1997), made parallel by collapsing an independent set of edges per round.  What the clustering simplifier above
 * cannot do: its output size follows from the grid alone.  Additive: NERF_ABI_VERSION stays 3.  All arithmetic is IEEE double, one
 * rounding per operation, in exactly the order and grouping written here; tests/_decimate_ref.py reproduces every output bit for bit.
 *   input     verts [V, 3] float32, colors [V, 3] float32 or NULL, faces [F, 3] int32; box lo[3] < hi[3] (host floats, finite);
 *             1 <= V, F <= 2^24.  ctr_a = ((double)lo_a + (double)hi_a) * 0.5; hs = max_a((double)hi_a - (double)lo_a) * 0.5.
 *             u_a = ((double)v_a - ctr_a) / hs: coordinates relative to the box centre, in units of half the longest side.  A
 *             vertex is finite when its three float32 coordinates are.
 *   state     across rounds: positions float32 [V, 3] (rounded once when written), per vertex the quadric Q of 10 doubles
 *             (Axx, Axy, Axz, Ayy, Ayz, Azz, bx, by, bz, c), a colour sum of 3 doubles (the float32 colours as doubles at first)
 *             and a merge count (1 at first); the face list.  Vertex indices are stable, vertices are compacted only at the end, in
 *             index order; faces are compacted every round, in input order.
 *   faces     a face with an index outside [0, V) is dropped before anything else and nothing is read through that index; so
 *             is a face with two equal corners.
 *   quadrics  for every face whose three corners are finite: e1 = u1 - u0, e2 = u2 - u0 (u0 the face's first corner),
 *             n = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x), d = -((nx u0x + ny u0y) + nz u0z),
 *             K = (nx nx, nx ny, nx nz, ny ny, ny nz, nz nz, nx d, ny d, nz d, d d): area^2-weighted.  Q[v] = the K of the faces
 *             of v added one by one to 0 in ascending face index -- the rows come from one sort of the 3 F keys
 *             (vertex << 27) | (face << 2) | corner, without atomics.  A fixed-order double sum: reproducible, and it DOES
 *             depend on the order of the faces.
 *   round 1. edges.  Corner c of face f gives the half-edge key (min << 25) | (max << 1) | (g_c > g_c+1) of (g_c, g_c+1).  In the
 *             sorted keys a run with one (min, max) is one edge (a, b), a < b; its rank among the runs is its id e.  A vertex is
 *             free iff it is finite and every edge at it is a run of exactly two half-edges of opposite direction.  Vertices on
 *             open, non-manifold or inconsistently oriented edges are frozen: this version never moves them.
 *         2. candidates.  Edge (a, b) is a candidate iff (i) both ends are free; (ii) the link condition holds: over the faces
 *             (a, n, p) at a and (b, n', p') at b, written from the end's corner on, n = n' for exactly two pairs (two common
 *             neighbours), and no face at a without b and face at b without a have {n, p} = {n', p'} (no ring edge is opposite both
 *             ends: what stops a tetrahedron collapsing to a double face); (iii) every face at a or b that does not hold both keeps
 *             dot > 0, dot = (n0x n1x + n0y n1y) + n0z n1z of its normal n0 = (p1 - p0) x (p2 - p0) (as n above) and the same
 *             with the moved corner at xbar.
 *             placement: q = Q[a] + Q[b]; m = (ua + ub) * 0.5; len2 = (dx dx + dy dy) + dz dz of d = ua - ub.  With
 *             NERF_DECIMATE_MIDPOINT, or when tr = (Axx + Ayy) + Azz <= 0: xbar = m.  Otherwise mu = (tr / 3) * 2^-10 and
 *             (A + mu I) x = mu m - b by Cramer's rule exactly as "mesh simplification" writes it out (a00 ... c22, det, x0, x1,
 *             x2 with r_a = mu m_a - b_a); x is taken when its three components are finite and
 *             (ex ex + ey ey) + ez ez <= len2 for e = x - m, else xbar = m.
 *             cost: Ax_0 = (Axx x0 + Axy x1) + Axz x2, Ax_1 = (Axy x0 + Ayy x1) + Ayz x2, Ax_2 = (Axz x0 + Ayz x1) + Azz x2;
 *             cost = ((x0 Ax_0 + x1 Ax_1) + x2 Ax_2 + 2 ((bx x0 + by x1) + bz x2)) + c, grouped as ((xAx) + (2 (b.x))) + c; 0
 *             unless cost > 0.  key = (the bits of (float)cost << 32) | ((e * 0x9E3779B1) mod 2^32).  The multiplier is odd, the
 *             low word a bijection of e: keys are unique, and exact cost ties -- the rule on coplanar marching-cubes faces -- do
 *             not order themselves along the vertex numbering.
 *         3. selection, `passes` times (1 <= passes <= 16); no vertex is blocked at first.  An edge takes part when it is a candidate and neither end
 *             is blocked.  m1[v] = the minimum key over the edges at v that take part (64-bit unsigned atomic minimum);
 *             m2[v] = min(m1[v], m1[u] over every edge (v, u)); an edge that takes part is selected iff its key equals m2[a] and
 *             m2[b].  Then every vertex that shares an edge with an end of a newly selected edge is blocked, the ends included.
 *             Independence: two selected edges of a round never share or adjoin a vertex.  In one pass: key(e) >= m1[a] >= m2[a]
 *             for an edge e at a that takes part, so a selected e has key(e) = m2 of both ends.  If selected e = (a, b) and e' = (c,
 *             d) shared a vertex v, key(e) = m2[v] = key(e'), and keys are unique: e = e'.  If an edge joined a to c,
 *             key(e) = m2[a] <= m1[c] <= key(e') and key(e') = m2[c] <= m1[a] <= key(e): again e = e'.  Across passes: a later
 *             edge takes part only with both ends unblocked, so neither is an end of an earlier selected edge or joined to one.
 *             A collapse of (a, b) reads and writes only a, b, their faces and their neighbours' positions; a face that holds an end
 *             of e and an end of e' would join them.  So every ring a collapse reads is untouched by the others, no collapse of
 *             the round creates an edge between two neighbours of a or b, and the round equals the same collapses done one after
 *             another in any order.
 *         4. trim.  With S selected edges and F faces, if F - 2 S < target only the k = ceil((F - target) / 2) smallest keys
 *             stay (one sort of the selected keys).  Every collapse removes exactly two faces (the link condition), so the result
 *             has `target` or `target - 1` faces.
 *         5. apply, one lane per selected edge, one writer per vertex: pos[a] = (float)(ctr + xbar * hs) per axis;
 *             Q[a] = Q[a] + Q[b], and so the colour sums and the merge counts; b becomes a in every face, faces with two equal
 *             corners are dropped, the face list is compacted in order (count -> scan -> write).
 *         6. one host read of (F', collapses, candidates, frozen vertices).  The caller stops when F <= target ("target"), when a
 *             round selected nothing ("selected nothing") or after max_rounds rounds ("max_rounds").
 *   finish    the vertices the faces use, in index order, with positions as they stand and colours (float)(sum_a / count);
 *             normals by the rule of "mesh smoothing" (nerf_smooth_build, nerf_smooth_normals on the output).
 * Calls, with the same (V, F) -- the input's -- and workspace throughout; F_cap >= the current face count bounds the launches
 * (the kernels take the face count itself from device memory), `list` (0 first, then alternating) names the current one of the two face lists:
 *   nerf_decimate_begin     the state and face list 0; totals int64 [1] = the faces that stay, read once by the caller.
 *   nerf_decimate_keys      keys int64 [2][3 F_cap]: the half-edge keys and the incidence keys, INT64_MAX behind the 3 F in use.
 *   (the caller)            each row sorted ascending (one sort along the last axis).
 *   nerf_decimate_edges     rows, edges, ranks, frozen flags.
 *   nerf_decimate_quadrics  the initial quadrics; once, behind the first nerf_decimate_edges.
 *   nerf_decimate_select    candidates and the passes; sel_keys int64 [3 F_cap]: the selected keys, INT64_MAX elsewhere.
 *   (the caller)            sel_keys sorted ascending.
 *   nerf_decimate_apply     trim, collapses, face remap into the other list; totals int64 [4] as in step 6.
 *   nerf_decimate_count     totals int64 [2] = (V', F') of the current list.
 *   nerf_decimate_write     verts_out [V', 3], colors_out [V', 3] or NULL, faces_out [F', 3]; nothing is written past V_out / F_out.
 * No float atomics; the only atomics are 64-bit integer minima, besides stores of equal values.  workspace:
 * nerf_decimate_workspace_bytes(V, F) bytes (-1 out of range), kept from begin to write; its content on entry is unspecified.
 * Out of range: NERF_E_SHAPE; NULL: NERF_E_NULL; all argument checks run before any device work.
 * Not done: collapsing boundary or non-manifold vertices, invariance to the face order, a geometric error bound as a stopping
 * rule, texture or UV carry-over, a multi-rank path.                                                                            */
#define NERF_DECIMATE_MIDPOINT 0
#define NERF_DECIMATE_QUADRIC 1
int64_t nerf_decimate_workspace_bytes(int64_t V, int64_t F);
int nerf_decimate_begin(const float* verts, const float* colors, int64_t V, const int32_t* faces, int64_t F, void* workspace,
                        int64_t* totals, void* stream);
int nerf_decimate_keys(int64_t V, int64_t F, int64_t F_cap, int list, void* workspace, int64_t* keys, void* stream);
int nerf_decimate_edges(int64_t V, int64_t F, int64_t F_cap, const int64_t* sorted_keys, void* workspace, void* stream);
int nerf_decimate_quadrics(int64_t V, int64_t F, int list, const float* lo_host, const float* hi_host, void* workspace, void* stream);
int nerf_decimate_select(int64_t V, int64_t F, int64_t F_cap, int list, const float* lo_host, const float* hi_host, int placement,
                         int passes, void* workspace, int64_t* sel_keys, void* stream);
int nerf_decimate_apply(int64_t V, int64_t F, int64_t F_cap, int list, const float* lo_host, const float* hi_host, int placement,
                        int has_colors, int64_t target, const int64_t* sorted_sel_keys, void* workspace, int64_t* totals,
                        void* stream);
int nerf_decimate_count(int64_t V, int64_t F, int64_t F_cap, int list, void* workspace, int64_t* totals, void* stream);
int nerf_decimate_write(int64_t V, int64_t F, int list, int has_colors, void* workspace, int64_t V_out, int64_t F_out,
                        float* verts_out, float* colors_out, int32_t* faces_out, void* stream);

/* ---------------------------------------------------------------- mesh distance (no reference counterpart)
 * How far one mesh is from another: points drawn on a surface in proportion to area, and for each point the closest point of
 * another mesh (the Metro measurement of Cignoni, Rocchini and Scopigno, 1998).  It changes no mesh.  Additive: NERF_ABI_VERSION
 * stays 3.  All arithmetic is IEEE float32, one rounding per operation (no contraction), in exactly the order and grouping written
 * here, unless it says double or int64; a / b and sqrt are correctly rounded; dot(x, y) = (x0 y0 + x1 y1) + x2 y2.
 * tests/_distance_ref.py reproduces every output bit for bit.
 *   input     verts [V, 3] float32, faces [F, 3] int32, 0 <= V, F <= 2^24; box lo[3] < hi[3] (host floats, finite);
 *             ext_a = (double)hi_a - (double)lo_a.
 *   valid     a face (a, b, c) is valid unless it has an index outside [0, V), a corner with a non-finite coordinate, or a cross
 *             product n = e1 x e2 = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x), e1 = b - a, e2 = c - a, whose three
 *             components are exactly zero.  Nothing is read through a bad index; an invalid face is never drawn and never the
 *             closest one, and dropping it from the input changes no output bit but the face numbers.
 *   weight    d = sqrt((nx nx + ny ny) + nz nz), the float32 doubled area.  U = max_a(ext_a)^2 (double), x = (double)d / U, x = 16
 *             unless x < 16 (an area that overflowed to inf or NaN takes the cap), w = max(1, (int64)rint(x * 2^34)) for a valid
 *             face (rint: to nearest, ties to even) and 0 for any other.  One unit is 2^-35 of the area of the box's largest
 *             face; 2^24 faces of at most 2^38 units stay below 2^63; a face spanning one cell of an R = 512 lattice has 2^16
 *             units.  cdf_f = w_0 + ... + w_f (int64, exact: no summation order enters), total = cdf_{F-1}.
 *   draws     for sample i of seed s, with mix64 the splitmix64 finaliser (z ^= z >> 30, z *= 0xBF58476D1CE4E5B9, z ^= z >> 27,
 *             z *= 0x94D049BB133111EB, z ^= z >> 31), all in uint64: key = mix64(s ^ mix64(i + 0x632BE59BD9B4E019)),
 *             r_j = mix64(key + (j + 1) 0x9E3779B97F4A7C15) for j = 0, 1, 2.  target = the high 64 bits of r_0 * total, in
 *             [0, total); the face is the first f with cdf_f > target (binary search), so P(f) = w_f / total up to 2^-64 total.
 *             A = r_1 >> 40, B = r_2 >> 40 (24 bits each); when A + B > 2^24 (the point lies beyond the diagonal) A = 2^24 - A,
 *             B = 2^24 - B; u1 = A 2^-24, u2 = B 2^-24 (exact), so u1, u2 >= 0 and u1 + u2 <= 1 without a square root.
 *             point_x = (a_x + u1 (b_x - a_x)) + u2 (c_x - a_x) per axis.
 *   distance  of point p to a valid face (a, b, c), C. Ericson, "Real-Time Collision Detection" 5.1.5: ab = b - a, ac = c - a,
 *             ap = p - a, bp = p - b, cp = p - c; d1 = dot(ab, ap), d2 = dot(ac, ap), d3 = dot(ab, bp), d4 = dot(ac, bp),
 *             d5 = dot(ab, cp), d6 = dot(ac, cp); vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4.  The closest point q
 *             is taken by the first test that holds:
 *               d1 <= 0 and d2 <= 0                          q = a
 *               d3 >= 0 and d4 <= d3                         q = b
 *               vc <= 0 and d1 >= 0 and d3 <= 0              v = d1 / (d1 - d3), q = a + v ab
 *               d6 >= 0 and d5 <= d6                         q = c
 *               vb <= 0 and d2 >= 0 and d6 <= 0              w = d2 / (d2 - d6), q = a + w ac
 *               va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0    w = (d4 - d3) / ((d4 - d3) + (d5 - d6)), q = b + w (c - b)
 *               otherwise                                    s = (va + vb) + vc, v = vb / s, w = vc / s, q = (a + v ab) + w ac
 *             (a comparison with a NaN is false), and D(p, f) = dot(p - q, p - q).
 *   result    over the valid faces whose D is not NaN, the smallest 64-bit key (bits of D) 2^32 + f: dist2 = the smallest D, face =
 *             the lowest index that attains it.  No such face: dist2 = +inf, face = -1.  A point with a non-finite coordinate:
 *             dist2 = NaN (0x7FC00000), face = -1.  The result is that of a scan over every face, for points inside the box and
 *             outside; the grid below only decides which faces are looked at.
 *   grid      G^3 cells over the box, 1 <= G <= 256; cell of a coordinate x on axis a: t = ((double)x - lo_a) * (G / ext_a),
 *             0 unless t > 0, G - 1 when t >= G, else (int)t.  A valid face is entered into every cell of the product of its three
 *             cell ranges [cell(min), cell(max)]: its bounding box clamped onto the grid.  G = 1 is the scan over every valid face.
 *   query     one lane per point: the shells of cells at Chebyshev radius r = 0, 1, ... around the cell of the point (clamped like
 *             any coordinate).  After a shell, m is the distance (double) from the point projected onto the box to the nearest
 *             plane of the block of visited cells that still has cells behind it; every face not yet seen is at least m away.  A
 *             float32 distance differs from the true one: the computed closest point lies within 64 * 2^-24 * S of the triangle,
 *             S the largest |coordinate| among the point, the valid faces' corners and the box, and the squared norm has a
 *             relative error below 2^-21.  The walk stops when m > slack = 2^-18 S and (m - slack)^2 (1 - 2^-20) is strictly
 *             greater than the best dist2, or when every cell has been visited.
 * Calls:
 *   nerf_surface_cdf       cdf [F] int64: weights, their workgroup sums, one scan, the inclusive sums in place.  No atomics.
 *                          workspace: nerf_surface_cdf_workspace_bytes(F) bytes (-1 out of range).  F = 0: nothing is launched.
 *   nerf_surface_sample    points [n, 3], face [n] of samples 0 .. n - 1 of `seed`; `total` is cdf[F - 1], read once by the caller
 *                          (the sampler's one host read, as the simplifier's).  One lane per sample, no atomics, no host read.
 *                          n = 0: nothing is launched.  total <= 0 or F = 0 with n > 0: NERF_E_SHAPE, "the mesh has no area".
 *   nerf_meshdist_count    entries per cell (one integer atomic per cell and face), the largest |coordinate| of a valid face
 *                          (integer atomic max on the bits), the exclusive scan of the cells; total_out [1] int64 (device): the
 *                          number of entries, which exceeds F when faces are large or the grid is fine.  The caller reads it once
 *                          and sizes `entries`; above 2^30 the build refuses ("use a coarser grid"), nothing is truncated.
 *   nerf_meshdist_build    entries [E] int32, E = that total: the face indices through per-cell cursors.  The order inside a cell
 *                          depends on the arrival order; no result does.  No sort.
 *   nerf_meshdist_query    dist2 [n], face [n] of a chunk of points [n, 3] against the index; the same mesh, box, grid, workspace
 *                          and entries as the build.  No host read, no atomics; the index is only read, so one build serves any
 *                          number of chunks.  n = 0: nothing is launched.
 * workspace (count, build, query): nerf_meshdist_workspace_bytes(F, grid) bytes (-1 for arguments out of range), kept from the
 * count on; its content on entry is unspecified.  No float atomics, one writer per output element: bit-reproducible and
 * independent of the order of the faces (face numbers aside).  Out of range (V, F outside [0, 2^24], grid outside [1, 256], n
 * outside [0, 2^30], lo >= hi or a non-finite corner): NERF_E_SHAPE; NULL: NERF_E_NULL; all argument checks run before any
 * device work.
 * Not done: no BVH (a grid walk grows with the cube of the distance to the nearest face), no signed distance, no
 * point-cloud-to-point-cloud entry, no closest point returned (the face and the distance are), no per-face normals.             */
int64_t nerf_surface_cdf_workspace_bytes(int64_t F);
int nerf_surface_cdf(const float* verts, int64_t V, const int32_t* faces, int64_t F, const float* lo_host, const float* hi_host,
                     void* workspace, int64_t* cdf, void* stream);
int nerf_surface_sample(const float* verts, int64_t V, const int32_t* faces, int64_t F, const int64_t* cdf, int64_t total, int64_t n,
                        uint64_t seed, float* points, int32_t* face, void* stream);
int64_t nerf_meshdist_workspace_bytes(int64_t F, int grid);
int nerf_meshdist_count(const float* verts, int64_t V, const int32_t* faces, int64_t F, const float* lo_host, const float* hi_host,
                        int grid, void* workspace, int64_t* total_out, void* stream);
int nerf_meshdist_build(const float* verts, int64_t V, const int32_t* faces, int64_t F, const float* lo_host, const float* hi_host,
                        int grid, void* workspace, int32_t* entries, int64_t E, void* stream);
int nerf_meshdist_query(const float* points, int64_t n, const float* verts, int64_t V, const int32_t* faces, int64_t F,
                        const float* lo_host, const float* hi_host, int grid, const void* workspace, const int32_t* entries,
                        int64_t E, float* dist2, int32_t* face, void* stream);

/* ---------------------------------------------------------------- mesh BVH (no reference counterpart)
 * A second index for the queries of "mesh distance": a bounding-volume hierarchy over the faces, whose cost follows the surface
 * near the query and not the empty space between (the grid walks (2 r + 1)^3 cells to reach a face r cells away), and the closest
 * point of a given face.  dist2 and face are those of "mesh distance", result: the bits of the scan over every face; validity, the
 * distance D(p, f) and the key (bits of D) 2^32 + f are the ones written there.  Additive: NERF_ABI_VERSION stays 3.
 * tests/_bvh_ref.py reproduces every output bit for bit.
 *   keys      for a valid face, m_a = ((double)min_a + (double)max_a) * 0.5 per axis, min and max over its three float32 corners;
 *             cell c_a = ((m_a - lo_a) / ext_a) * 4096 in double, 0 unless it is > 0, 4095 when it is >= 4096, else truncated; the
 *             code is the 36-bit interleave (bit 3 i + a of the code = bit i of c_a: x lowest), an invalid face has code 2^36;
 *             key_f = code 2^24 + f (int64).  Keys are unique, so sorting them leaves nothing to the sort's stability.
 *   tree      the caller sorts the keys ascending.  A leaf holds LEAF = 4 consecutive sorted faces: nL = ceil(F / 4) leaves, P the
 *             smallest power of two >= max(nL, 1).  A complete binary tree in heap order: the root is node 1, the children of i
 *             are 2 i and 2 i + 1, the leaves are P .. 2 P - 1 (leaf P + j holds the sorted faces 4 j .. 4 j + 3), node 0 is unused.
 *             A node is six floats, the exact min and max of the float32 corner coordinates of the valid faces below it; a node
 *             with none is (+inf, -inf).  order [F]: the face of each sorted key, -1 for an invalid one.  The depth is at most 22.
 *   query     one lane per point, a stackless depth-first walk: the lane keeps the node index and one 32-bit trail word with a
 *             bit per level at which the far sibling is still pending.  At an internal node the child whose box is nearer is
 *             entered first (the left one on a tie); going up, the lane pops to the lowest set bit k, the pending sibling is
 *             (node >> k) ^ 1, and it is tested again, for the best distance may have improved.  A leaf takes D(p, f) of each of
 *             its valid faces into the smallest key.  Neither the order of the walk nor the tree enters the result.
 *   rule      m is the distance (double) from the point to a node's box; S the largest |coordinate| among the point, the root box
 *             and the box [lo, hi]; slack = 2^-18 S.  A node is skipped only if it is empty, or if m > slack and
 *             (m - slack)^2 (1 - 2^-20) is strictly greater than the best dist2.  Every point of a face lies in the boxes of all
 *             its ancestors, so m bounds the true distance from below; the slack and the factor cover the float32 error of the
 *             computed distance as in "mesh distance", query.  On equality a node is entered: a lower face index may still tie.
 *   closest   for point i and face f = face[i]: the q of "mesh distance", distance, as computed, so that dot(p - q, p - q) is dist2
 *             bit for bit when f is the face the query answered; three NaN (0x7FC00000) for f = -1, f outside [0, F) or an invalid
 *             face.
 * Calls:
 *   nerf_bvh_keys          keys [F] int64.  One lane per face, no atomics.  F = 0: nothing is launched.
 *   nerf_bvh_build         sorted_keys [F] int64 (the keys sorted ascending; every face named by a key is tested again, so keys
 *                          that are not this mesh's cannot lead a read out of range) -> the nodes and the order in the workspace:
 *                          one launch for the leaves, one per level upward, the levels of at most 256 nodes in one launch of one
 *                          workgroup; 2 + max(0, log2 P - 9) launches, at most 15, a function of F alone.  No atomics, no host
 *                          read, no workgroup waits for another.  F = 0: an empty root is written.
 *   nerf_bvh_query         dist2 [n], face [n] of a chunk of points [n, 3]; the same mesh and workspace as the build, and the box
 *                          (it enters S only).  No host read, no atomics, no LDS; the workspace is only read, so one build serves
 *                          any number of chunks.  n = 0: nothing is launched.
 *   nerf_closest_points    closest [n, 3] of points [n, 3] and face [n] int32.  Needs no index.  n = 0: nothing is launched.
 * workspace (build, query): nerf_bvh_workspace_bytes(F) bytes (-1 for an F out of range), starting on a multiple of 16 bytes:
 * the nodes [2 P][6] float32, then the order [F] int32, each region padded to 16 bytes.  Its content on entry is unspecified.  One
 * writer per output element: bit-reproducible; under a renumbering of the faces dist2 is unchanged and face follows the renumbering.
 * Out of range (V, F outside [0, 2^24], n outside [0, 2^30], lo >= hi or a non-finite corner, a misaligned workspace):
 * NERF_E_SHAPE; NULL: NERF_E_NULL; all argument checks run before any device work.
 * Not done: no surface-area-heuristic or Karras (longest-common-prefix) splits -- the tree is the implicit median split of the
 * Morton order; no signed distance; no ray casting (see mesh ray casting).                                                        */
int64_t nerf_bvh_workspace_bytes(int64_t F);
int nerf_bvh_keys(const float* verts, int64_t V, const int32_t* faces, int64_t F, const float* lo_host, const float* hi_host,
                  int64_t* keys, void* stream);
int nerf_bvh_build(const float* verts, int64_t V, const int32_t* faces, int64_t F, const int64_t* sorted_keys, void* workspace,
                   void* stream);
int nerf_bvh_query(const float* points, int64_t n, const float* verts, int64_t V, const int32_t* faces, int64_t F,
                   const float* lo_host, const float* hi_host, const void* workspace, float* dist2, int32_t* face, void* stream);
int nerf_closest_points(const float* points, int64_t n, const float* verts, int64_t V, const int32_t* faces, int64_t F,
                        const int32_t* face, float* closest, void* stream);

/* ---------------------------------------------------------------- mesh winding number (no reference counterpart)
 * On which side of a mesh a point lies: the generalized winding number (Jacobson, Kavan and Sorkine-Hornung 2013), summed over
 * the hierarchy of "mesh BVH" with far subtrees replaced by their dipole (Barill, Dickson, Schmidt, Levin and Jacobson 2018, the
 * first-order term).  It is defined for open, duplicated and self-intersecting meshes: 1 inside a closed mesh whose faces are
 * counter-clockwise seen from outside (n = (b - a) x (c - a) points outward, the orientation of "mesh extraction"), 0 outside,
 * and in between near a hole.  It changes no mesh.  Additive: NERF_ABI_VERSION stays 3.  All arithmetic is IEEE double on the
 * float32 corners a, b, c and the float32 point q, one rounding per operation (no contraction), in exactly the order written
 * here; dot(u, v) = (u0 v0 + u1 v1) + u2 v2 and u x v = (u1 v2 - u2 v1, u2 v0 - u0 v2, u0 v1 - u1 v0).  tests/_winding_ref.py follows
 * it operator for operator; the one operation a device may round differently is atan2.  Validity of a face is that of "mesh
 * distance".
 *   exact     x = a - q, y = b - q, z = c - q; lx = sqrt(dot(x, x)), ly, lz alike; det = dot(x, y x z);
 *             den = (((lx ly) lz + dot(x, y) lz) + dot(y, z) lx) + dot(z, x) ly; Omega = 2 atan2(det, den), and Omega = 0 where
 *             det == 0: q lies in the plane of the face.  w = (sum of Omega) / (4 pi), 4 pi = 12.566370614359172.  Inside is
 *             w > 0.5.  The value at a point of the surface itself is this convention and nothing more.
 *   moments   one record of 12 doubles per node of the hierarchy, heap order: N [0..2], c [3..5], r [6], A [7], S [8..10], 0.  A
 *             leaf starts from zeros and visits its valid faces in sorted order: n_f = 0.5 ((b - a) x (c - a)), a_f =
 *             sqrt(dot(n_f, n_f)); N += n_f; S_k += (a_f ((a_k + b_k) + c_k)) / 3; A += a_f.  An internal node is left + right,
 *             in that order, for N, S and A.  c = S / A, and where A == 0 the midpoint ((double)min + (double)max) 0.5 of the
 *             node's box; e_k = fmax(c_k - min_k, max_k - c_k), r = sqrt(dot(e, e)): from c to the farthest corner of the node's
 *             float32 box.  A node without a valid face, and node 0, are twelve zeros.
 *   query     one lane per point, stackless, no trail word: the lane keeps the node index alone, and the order of the sum is
 *             fixed.  Start at node 1.  An empty node (min > max) is skipped.  A leaf adds Omega of each of its valid faces in
 *             sorted order.  An internal node with d = c - q, d2 = dot(d, d) adds the dipole dot(N, d) / (d2 sqrt(d2)) iff
 *             d2 > (beta beta) (r r), strictly and in double, so that a NaN product never approximates; otherwise the walk
 *             descends to the left child 2 i.  Next: while the node is odd, halve it; stop at 0 (so also on reaching 1 again);
 *             otherwise add 1.  beta = +inf is the exact sum in the tree's order.
 *   result    w [n] float64; visits [n, 2] int32 = (faces evaluated exactly, nodes approximated).  A point with a non-finite
 *             coordinate: (NaN 0x7FF8000000000000, 0, 0).  A mesh without a valid face: (0, 0, 0).
 * Calls:
 *   nerf_winding_build     the moments from a built hierarchy (bvh_workspace: what nerf_bvh_build wrote for this mesh; every face
 *                          its order names is tested again): one launch for the leaves, one per level upward, the levels of at
 *                          most 256 nodes in one launch of one workgroup: nerf_bvh_build's count, a function of F alone.  No
 *                          atomics, no LDS, no host read, no workgroup waits for another.  F = 0: nothing is launched.
 *   nerf_winding_query     w [n], visits [n, 2] of a chunk of points [n, 3]; beta a double >= 1 or +inf.  Both workspaces are only
 *                          read, so one build serves any number of chunks, and no result depends on the chunking.  n = 0:
 *                          nothing is launched.
 * workspace (build, query): nerf_winding_workspace_bytes(F) bytes (-1 for an F out of range) = 2 P 96, starting on a multiple of
 * 16 bytes; its content on entry is unspecified.  One writer per output element: bit-reproducible.
 * Out of range (V, F outside [0, 2^24], n outside [0, 2^30], a beta that is NaN or below 1, a misaligned workspace):
 * NERF_E_SHAPE; NULL: NERF_E_NULL; all argument checks run before any device work.
 * Not done: no quadrupole or higher terms (the dipole's error at beta = 2 is about 0.015 of a turn); no narrow band, so every
 * lattice point of a volume is evaluated; no culling of faces that lie inside the solid; still no ray casting (see
 * mesh ray casting).                                                                                                              */
int64_t nerf_winding_workspace_bytes(int64_t F);
int nerf_winding_build(const float* verts, int64_t V, const int32_t* faces, int64_t F, const void* bvh_workspace, void* workspace,
                       void* stream);
int nerf_winding_query(const float* points, int64_t n, const float* verts, int64_t V, const int32_t* faces, int64_t F,
                       const void* bvh_workspace, const void* workspace, double beta, double* w, int32_t* visits, void* stream);

/* ---------------------------------------------------------------- mesh ray casting (no reference counterpart)
 * Where a ray meets a mesh: the nearest hit, or whether there is one, on the hierarchy of "mesh BVH".  The rays are the rows
 * nerf_ray_gen writes for the field, unchanged: rays [n, NERF_RAY_STRIDE] float32 with o in columns 0-2, d in 3-5 (not normalised:
 * t counts in units of d), tmin in 6, tmax in 7; columns 8-10 are not read.  It changes no mesh.  Additive: NERF_ABI_VERSION stays 3.
 * All arithmetic of the face test and of the box test is IEEE double on the float32 corners and rays, one rounding per operation
 * (no contraction), in exactly the order written here; a / b is correctly rounded, and so are the casts to float32.
 * tests/_raycast_ref.py follows it operator for operator.  Validity of a face is that of "mesh distance".
 *   ray       valid iff o and d are finite, d != 0, tmin and tmax are not NaN and tmin >= 0 (tmax = +inf is allowed).  Any other
 *             ray answers t = NaN (0x7FC00000), face = -1, bary = (NaN, NaN), visits = (0, 0), hit = 0.  tmin > tmax is a valid ray
 *             that misses.
 *   frame     (Woop, Benthin and Wald 2013) kz is the axis of the largest |d_a|, the lowest axis on a tie; kx = (kz + 1) mod 3 and
 *             ky = (kx + 1) mod 3, swapped if d[kz] < 0.  Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz].
 *   face      for the corners a, b, c: A = a - o per component; Ax = A[kx] - Sx A[kz], Ay = A[ky] - Sy A[kz], Az = Sz A[kz]; B and
 *             C alike.  U = Cx By - Cy Bx, V = Ax Cy - Ay Cx, W = Bx Ay - By Ax.  The ray misses the face if one of U, V, W is < 0
 *             while another is > 0 (zeros are inclusive).  det = (U + V) + W; det == 0 misses.  t64 = ((U Az + V Bz) + W Cz) / det;
 *             t = (float)t64 + 0.0f (a -0 becomes +0); the hit is accepted iff tmin <= t and t <= tmax, compared in float32.
 *             bary = ((float)(V / det), (float)(W / det)): the weights of the second and third corner, as "mesh rendering" and
 *             nerf_texture_sample take them.
 *   edges     the edge function of the edge (p, q) is px qy - py qx up to its sign, whatever face it is computed for and in
 *             whichever order the face lists p and q: the same two products (a product does not depend on the order of its
 *             factors), subtracted one way or the other, so the two faces that share an edge get values that are exact negatives
 *             of each other.  A ray that passes through the shared edge of two faces of a closed, consistently oriented surface
 *             therefore sees 0 in both, or a value on the inner side of one of them: no ray slips between them.
 *   result    nerf_raycast answers the minimum over all valid faces of the key (bits of t) 2^32 + f among the accepted hits: the
 *             nearest hit, the lowest face index on equal t.  t [n] float32, face [n] int32, bary [n, 2] float32 of that face,
 *             visits [n, 2] int32 = (faces tested, boxes tested).  A miss: (+inf, -1, NaN, NaN).  Neither the order of the walk
 *             nor the shape of the tree enters t, face or bary; visits is a function of the tree and the ray alone.
 *             nerf_raycast_any answers hit [n] uint8 = 1 iff nerf_raycast would answer face >= 0; its walk stops at the first
 *             accepted hit.
 *   walk      that of "mesh BVH", query: one lane per ray, stackless, the node index and one 32-bit trail word.  At an internal
 *             node both children are read (three 16-byte words) and tested; of two that stay, the one whose entry parameter is
 *             smaller is entered first (the left one on a tie) and the other is marked pending; going up, the lane pops to the
 *             lowest set bit k, the pending sibling is (node >> k) ^ 1, and it is tested again, for the best hit may have come
 *             nearer.  A leaf tests each of its valid faces in sorted order.  boxes tested counts the root (once), two per
 *             internal node entered and one per pop; faces tested counts the face tests.
 *   box       S is the largest |coordinate| among the ray's origin, the root box and the box [lo, hi]; eta = 2^-30 S.  A node
 *             (min, max) is widened to lo_a = (double)min_a - eta, hi_a = (double)max_a + eta.  Per axis with d_a != 0:
 *             inv_a = 1 / d_a, t0 = (lo_a - o_a) inv_a, t1 = (hi_a - o_a) inv_a, swapped if inv_a < 0; enter = the largest t0,
 *             exit = the smallest t1 (starting from -inf and +inf).  An axis with d_a == 0 has no parameters (no 0 inf is ever
 *             formed): it only asks whether lo_a <= o_a <= hi_a.  The line meets the widened box iff every such axis says yes and
 *             enter <= exit.
 *   rule      a node is skipped only if it is empty (min > max), or the line does not meet its widened box, or
 *             (float)exit < tmin, or (float)enter > tmax, or (float)enter is strictly greater than the best t.  On equality
 *             with the best t the node is entered: a lower face index may still tie.
 *   proof     Let a face below the node be accepted with U, V, W >= 0 (or all <= 0) and det != 0.  (1) Along kz: rounding is
 *             monotone, so Az = fl(Sz fl(a_kz - o_kz)) lies, for every corner, between the node's own t0 and t1 of that axis
 *             (the same two operations on min_kz - eta and max_kz + eta, and inv_kz is Sz).  The products U Az, V Bz, W Cz have
 *             weights of one sign, so t64 is a convex combination of Az, Bz, Cz up to five roundings: |t64 - c| <= 2^-49 M with
 *             M = max |Az, Bz, Cz| <= 2 S |Sz|, while the widening moved t0 and t1 outward by eta |Sz| = 2^-30 S |Sz|, 2^18 times
 *             as much.  So t0 <= t64 <= t1 on the axis kz whatever the shape of the face.  (2) Across: U A' + V B' + W C' = 0 holds
 *             exactly for the exact edge functions of the sheared corners A' = (Ax, Ay), ..., so with the computed ones, each
 *             within 2^-51 R^2 of exact (two products and a difference of numbers below R^2, R <= 4 S the largest sheared
 *             coordinate, |Sx|, |Sy| <= 1), the sheared origin lies inside the sheared triangle or outside it by no more than
 *             2^-48 R, unless the three sheared corners are themselves collinear with the origin to that relative precision (see
 *             Not done).  The sheared coordinates of a point are its offsets from the ray's point of the same kz, so the ray
 *             passes within 2^-46 S of a point P of the face at the parameter c, and P lies in every ancestor's box.  With (1),
 *             the ray's point at t64 is within 2^-45 S of the box on every axis; each computed t0, t1 is the exact parameter of
 *             a plane moved by at most 2^-50 S (two roundings of numbers below 2 S); together far inside eta.  Hence
 *             enter <= t64 <= exit as computed, and, the cast to float32 being monotone (and + 0.0f changing no order),
 *             (float)enter <= t <= (float)exit.  A node skipped by the rule has (float)enter > min(tmax, best t) or
 *             (float)exit < tmin, so no face below it can be accepted with a key at or below the best.  tests/_raycast_ref.py
 *             emulates the walk and holds it to the scan over every face bit for bit.
 * Calls:
 *   nerf_raycast           t [n], face [n], bary [n, 2], visits [n, 2] of a chunk of rays [n, 11]; the mesh and the box of the
 *                          build (the box enters S only); bvh_workspace: what nerf_bvh_build wrote for this mesh.  One lane per
 *                          ray; no atomics, no LDS, no scratch, no host read, no workgroup waits for another.  The workspace is
 *                          only read and there is no other: one build serves any number of chunks, and no result depends on the
 *                          chunking or the launch shape.  n = 0: nothing is launched.
 *   nerf_raycast_any       hit [n] uint8 of the same arguments.  n = 0: nothing is launched.
 * One writer per output element: bit-reproducible; under a renumbering of the faces t and bary are unchanged where the nearest
 * hit is on one face only, and face follows the renumbering.
 * Out of range (V, F outside [0, 2^24], n outside [0, 2^30], lo >= hi or a non-finite corner, a misaligned workspace):
 * NERF_E_SHAPE; NULL: NERF_E_NULL; all argument checks run before any device work.
 * Not done: no all-hits or parity counting (an inside test by crossings: "mesh winding number" is the inside test); no agreement
 * with the rasteriser that is exact at the near plane (a face that crosses it is cut here and dropped there) or at silhouettes
 * (it snaps to 1/256 pixel); no packet or wave-cooperative traversal (one lane per ray, divergent lanes wait for each other); no
 * better splits than the Morton median; a face that the ray sees exactly edge-on to double precision, its sheared corners
 * collinear with the ray, is outside the proof of the rule (exactly edge-on it has det == 0 and misses).                          */
int nerf_raycast(const float* rays, int64_t n, const float* verts, int64_t V, const int32_t* faces, int64_t F, const float* lo_host,
                 const float* hi_host, const void* bvh_workspace, float* t, int32_t* face, float* bary, int32_t* visits, void* stream);
int nerf_raycast_any(const float* rays, int64_t n, const float* verts, int64_t V, const int32_t* faces, int64_t F,
                     const float* lo_host, const float* hi_host, const void* bvh_workspace, uint8_t* hit, void* stream);

/* ---------------------------------------------------------------- texture atlas (no reference counterpart)
 * A texture for a finished mesh, baked by one field query per texel: a simplified mesh then carries the field's appearance at
 * a resolution of its own, not one colour per surviving vertex.  A separate step behind the export pipeline; it changes no
 * mesh.  Additive: NERF_ABI_VERSION stays 3.  All arithmetic is IEEE float32, one rounding per operation (no contraction), in
 * exactly the order and grouping written here; a / b and sqrt are correctly rounded; pos(x) = x > 0 ? x : 0 and
 * unit(x) = min(pos(x), 1) send NaN to 0.  tests/_texture_ref.py reproduces every output bit for bit.
 *   input     verts, normals [V, 3] float32, faces [F, 3] int32, 0 <= V, F <= 2^24; texels T, an int in [2, 64].
 *   layout    every face gets a right triangle of T texels a leg; two faces share a square cell of side S = T + 2.
 *             cells = ceil(F / 2); C = the smallest integer >= 1 with C C >= cells; W = C S, H = max(1, ceil(cells / C)) S; both
 *             at most NERF_TEXTURE_MAX_SIDE, else NERF_E_SHAPE with a text that names the largest T that fits.  Atlas texel
 *             (X, Y), Y the image row and row 0 the top one, raster index p = X + W Y (int64), lies in cell
 *             c = (Y / S) C + X / S at (i, j) = (X mod S, Y mod S).  It belongs to face 2c if i + j <= S - 1; otherwise to face
 *             2c + 1, and (i, j) becomes (S - 1 - i, S - 1 - j).  A texel whose face is >= F is unused.
 *   corners   face (a, b, c) has a at the centre of its local texel (0, 0), b at (T - 1, 0), c at (0, T - 1).  Local texel (i, j)
 *             has the barycentrics wb = (float)i / (float)(T - 1), wc = (float)j / (float)(T - 1), wa = (1 - wb) - wc.  wa is not
 *             clamped: the texels beyond the hypotenuse (the gutter) lie in the face's plane at extrapolated positions, so a
 *             bilinear lookup of a field that is affine in position reproduces it up to the 8-bit quantisation.  Every texel
 *             with a non-zero weight in a bilinear lookup inside a face's UV triangle belongs to that face, up to rounding
 *             on the hypotenuse: the float32 products of `sample` can put a point of it one ulp outside, and the diagonal
 *             texel of the cell's other face then gets a weight of order 1e-14.
 *   bad face  a face with an index outside [0, V) gets zero rows and black texels; nothing is read through the index, and
 *             nothing is read on the host to find such faces.
 *   row       position x = (wa A + wb B) + wc C per axis; direction m = (pos(wa) nA + pos(wb) nB) + pos(wc) nC from the vertex
 *             normals, len = sqrt((mx mx + my my) + mz mz), n = m / len when 0 < len < inf, else 0.  The row is
 *             [x, -n, 0, 0, -n], the colour query row of nerf_mesh_write_vertices; the row of an unused texel or of a bad face
 *             is eleven +0.
 *   colour    byte = (uint8)rint(255 unit(c)) for the first three of the four floats the query returned for the texel; 0 for
 *             an unused texel or a bad face whatever raw holds.
 *   uv        the corner at atlas texel (X, Y): u = ((float)X + 0.5f) / (float)W, v = 1.0f - ((float)Y + 0.5f) / (float)H
 *             (OBJ's convention: v goes up).
 *   sample    (face, wb, wc): wb = unit(wb); wc = min(pos(wc), 1 - wb).  A face outside [0, F) gives rgb 0 and a zero row.  Local
 *             texel coordinates x = wb (float)(T - 1), y = wc (float)(T - 1); i0 = (int)floor(x) clamped to [0, S - 2], j0
 *             likewise, fx = x - (float)i0, fy = y - (float)j0; with gx = 1 - fx, gy = 1 - fy the weights are w00 = gx gy,
 *             w10 = fx gy, w01 = gx fy, w11 = fx fy (the first index along i), c = (float)byte / 255.0f, and per channel
 *             rgb = ((w00 c00 + w10 c10) + w01 c01) + w11 c11.  The optional row is that of `row` at (wb, wc).
 * Calls:
 *   nerf_texture_layout    host only: out = {W, H, C, S}.  Needs no device.
 *   nerf_texture_rows      rows [count, 11] of the texels [p0, p0 + count) of the atlas in raster order, one lane per texel.
 *   nerf_texture_store     image [H, W, 3] uint8 for the same texels from raw [count, 4] (16-byte aligned), one lane per texel;
 *                          the bytes of other texels are not touched, so the image does not depend on how the atlas is cut
 *                          into chunks.
 *   nerf_texture_uv        uv [F, 3, 2], one lane per face.
 *   nerf_texture_sample    rgb [n, 3] and, when `rows` is not NULL, rows [n, 11] of n < 2^31 samples sample_face [n] int32,
 *                          bary [n, 2] = (wb, wc); verts, normals and faces are read for the rows only.
 * No atomics, no workspace, no host read; every output element has one writer: bit-reproducible.  Out of range: NERF_E_SHAPE;
 * NULL: NERF_E_NULL; all argument checks run before any device work.  count = 0, n = 0, F = 0 (uv): nothing is launched.
 * Not done: no mipmaps in this section (one atlas is safe for bilinear filtering at level 0 only; "texture mip pyramid" builds
 * the coarser levels), no chart packing by area (every face gets the same texels whatever its size), no seam handling across
 * face edges beyond the shared field.                                                                                            */
#define NERF_TEXTURE_MAX_SIDE 16384
int nerf_texture_layout(int64_t F, int texels, int64_t* out_host);
int nerf_texture_rows(const float* verts, const float* normals, int64_t V, const int32_t* faces, int64_t F, int texels, int64_t p0,
                      int64_t count, float* rows, void* stream);
int nerf_texture_store(const float* raw, int64_t V, const int32_t* faces, int64_t F, int texels, int64_t p0, int64_t count,
                       uint8_t* image, void* stream);
int nerf_texture_uv(int64_t F, int texels, float* uv, void* stream);
int nerf_texture_sample(const uint8_t* image, const float* verts, const float* normals, int64_t V, const int32_t* faces, int64_t F,
                        int texels, const int32_t* sample_face, const float* bary, int64_t n, float* rgb, float* rows, void* stream);

/* ---------------------------------------------------------------- mesh rendering (no reference counterpart)
 * A visibility-buffer rasteriser: what a posed pinhole camera sees of a finished mesh, so that an exported mesh can be compared
 * in image space with the held-out frame and with the field's own render.  Additive: NERF_ABI_VERSION stays 3.  Float steps are
 * IEEE float32, one rounding per operation (no contraction), in exactly the order and grouping written here, a / b correctly
 * rounded; integer steps are exact.  csrc/raster.h states the rule in code; tests/_raster_ref.py reproduces every output bit for
 * bit.
 *   input     verts [V, 3] float32, faces [F, 3] int32, 0 <= V, F <= 2^24; image 1 <= H, W <= 16384; near finite and > 0; the
 *             camera a nerf_tsdf_view on the host.
 *   camera    per vertex p, `point` and then `pixel` of "pinhole camera" (the tests below follow the division).  Depth is zc.
 *   snap      X = (int)rintf(u * 256.0f), Y = (int)rintf(v * 256.0f): screen coordinates in 1 / 256 pixel.
 *   dropped   a face is dropped and counted, never clipped: an index outside [0, V) or a non-finite vertex coordinate ("other";
 *             nothing is read through a bad index); else a vertex with !(near <= zc < inf), or with !(|u| <= 2^20) or
 *             !(|v| <= 2^20), the guard band, compared as floats before the cast ("depth or guard band"); else D = 0, or D > 0
 *             with cull_backfaces ("other"), where D = (Xb - Xa)(Yc - Ya) - (Yb - Ya)(Xc - Xa) in int64.  v grows downwards, so
 *             a face that is counter-clockwise seen from the camera, a front face of "mesh extraction", has D < 0.  The guard
 *             band keeps |X|, |Y| <= 2^28: a coordinate difference is below 2^30, a product of two below 2^59, D and every edge
 *             function below 2^60.
 *   coverage  s = sign(D), S = s D > 0.  E(U, V; P) = (Vx - Ux)(Py - Uy) - (Vy - Uy)(Px - Ux) at P = (256 px, 256 py);
 *             Ea = s E(B, C; P), Eb = s E(C, A; P), Ec = s E(A, B; P); Ea + Eb + Ec = S exactly.  Pixel (px, py) is covered iff
 *             Ea >= 0, Eb >= 0 and Ec >= 0 (inclusive).  E(U, V; P) = -E(V, U; P) exactly, so a pixel centre on an edge shared
 *             by two faces belongs to both and a closed surface has no cracks; the key decides between them.
 *   pixel     per covered pixel and face: qa = (float)Ea / za, qb = (float)Eb / zb, qc = (float)Ec / zc (int64 -> float32
 *             rounds to nearest even); Q = (qa + qb) + qc; wb = qb / Q; wc = qc / Q; z = (float)S / Q.  Perspective-correct:
 *             1 / z is the screen-space interpolation of 1 / zc.
 *   key       ((uint64)bits(z) << 32) | (uint32)(face_base + face index), one 64-bit atomicMin per covered pixel on keys
 *             uint64 [H W], pixel index px + W py.  A cleared pixel holds all ones.  z > 0, so its bits order like its value; of
 *             equal depths the lower face id wins.  A minimum does not depend on the order of its operands: the buffer is
 *             bit-reproducible and independent of face order, launch shape, small_max and of how a mesh is cut into draws.
 *             No float atomics.
 *   stats     uint64 [4]: faces drawn (not dropped, whether or not they cover a pixel), faces dropped for depth or guard band,
 *             faces dropped for another reason, key updates attempted = covered (pixel, face) pairs.
 *   resolve   per pixel: empty (key all ones): face -1, bary (0, 0), depth 0, acc 0.  Otherwise the winner's setup and `pixel`
 *             again, which gives the bits of the draw: face int32 = the id, bary float32 (wb, wc), the pair nerf_texture_sample
 *             takes, depth = z, acc = 1.  depth and acc are a renderer's aux maps of an opaque surface (depth / acc = zc):
 *             nerf_tsdf_integrate takes them unchanged.  An id outside [0, F) or a winner the setup refuses reads as empty.
 *   shade     per pixel with face >= 0: rgb_in's pixel if rgb_in is given (what the caller looked up, e.g. nerf_texture_sample
 *             at (face, bary)); else with wa = (1 - wb) - wc per channel (wa ca + wb cb) + wc cc of the vertex colours [V, 3]
 *             (a face outside [0, F) or with an index outside [0, V): the background).  face < 0: the background, one colour
 *             [3] or, with per_pixel, [H W, 3] (device memory).
 * Calls:
 *   nerf_raster_clear      keys to all ones and stats to 0, one lane per pixel.
 *   nerf_raster_draw       faces [F, 3] with ids face_base + f (0 <= face_base <= 2^24 - F) into keys; adds to stats.  It does
 *                          not clear: several meshes or chunks of faces share a buffer.  One lane per face does the setup and
 *                          the bounding box of the snapped corners clipped to the image, the pixels with X_min <= 256 px <= X_max
 *                          and Y_min <= 256 py <= Y_max inside [0, W) x [0, H).  A face whose box has at most small_max
 *                          pixels (0 <= small_max <= 2^30) is walked by its own lane; the others one after another by the
 *                          whole wave.  0: every face by the wave; 2^30: every face by its lane.  The keys and the stats do
 *                          not depend on it.  NERF_RASTER_SMALL_MAX is the measured default.  F = 0 launches nothing.
 *   nerf_raster_resolve    face [H W] int32, bary [H W, 2], depth [H W], acc [H W] from keys; faces is the whole array the ids
 *                          index.
 *   nerf_raster_shade      rgb [H W, 3]; exactly one of colors and rgb_in is not NULL.
 * Out of range: NERF_E_SHAPE; NULL: NERF_E_NULL; all argument checks run before any device work; nothing is read on the host.
 * Not done: no near-plane clipping (a face with a vertex in front of `near` is dropped: the project's cameras stand outside
 * the scene box), no antialiasing or supersampling (one sample at the pixel centre, like one ray per pixel), no mipmapped
 * texture lookups in these calls (nerf_mip_sample of "texture mip pyramid" has them), no tile binning for screen-filling
 * faces, no transparency.                                                                                                        */
#define NERF_RASTER_SMALL_MAX 16
int nerf_raster_clear(uint64_t* keys, int H, int W, uint64_t* stats, void* stream);
int nerf_raster_draw(const float* verts, int64_t V, const int32_t* faces, int64_t F, int64_t face_base,
                     const nerf_tsdf_view* view_host, int H, int W, float near, int cull_backfaces, int small_max, uint64_t* keys,
                     uint64_t* stats, void* stream);
int nerf_raster_resolve(const uint64_t* keys, const float* verts, int64_t V, const int32_t* faces, int64_t F,
                        const nerf_tsdf_view* view_host, int H, int W, float near, int32_t* face, float* bary, float* depth,
                        float* acc, void* stream);
int nerf_raster_shade(const int32_t* face, const float* bary, const int32_t* faces, int64_t V, int64_t F, const float* colors,
                      const float* rgb_in, const float* background, int per_pixel, int H, int W, float* rgb, void* stream);

/* ---------------------------------------------------------------- fused renderer (a14 / a18)
 * replaces: rendering/render.py:164-241 render_rays_eval (coarse pass, importance sampling, sort, second pass)
 * as ONE call that enqueues the fixed kernel sequence on `stream`: nerf_sample_coarse -> nerf_query_fused ->
 * nerf_composite_forward -> nerf_importance_sample -> nerf_query_fused -> nerf_composite_forward.
 * workspace: nerf_render_workspace_bytes(B,n,N) bytes of scratch.  packed_fine NULL = network_coarse
 * (render.py:228).  N == 0: coarse result only.  Optional outputs may be NULL.  u [B,N] = the uniforms that
 * sampling/__init__.py:140 draws with torch.rand.                                                          */
int64_t nerf_render_workspace_bytes(int64_t B, int n, int N);
int nerf_render_rays_fused(const nerf_mlp_arch* arch, const void* packed_coarse, const void* packed_fine,
                           const float* rays, int64_t B, int n, int N, const float* u, int freq_mode, int white_bkgd,
                           void* workspace, float* rgb, float* disp, float* acc, float* rgb_coarse, float* disp_coarse,
                           float* acc_coarse, float* z_vals, float* weights, void* stream);

/* ---------------------------------------------------------------- view-projected texture (no reference counterpart)
 * The atlas of "texture atlas" coloured from posed images, as photogrammetry pipelines bake a texture: every texel is projected
 * into every view, the observation is kept only where the mesh's own depth map of that view ("mesh rendering") says the texel is
 * visible, and the observations are blended.  The texels then hold what cameras saw along their rays, not what the field answers
 * along minus the normal.  Additive: NERF_ABI_VERSION stays 3.  All float steps are IEEE float32, one rounding per operation (no
 * contraction), in exactly the order and grouping written here; a / b and sqrt are correctly rounded.  csrc/project.h states the
 * rule in code; tests/_project_ref.py reproduces every output bit for bit.
 *   input     the mesh, texels T and the atlas of "texture atlas"; n <= NERF_PROJECT_MAX_VIEWS views, each a nerf_tsdf_view on the
 *             host, an image [H, W, 3] float32 and a depth / acc map pair [H W] float32 of the same camera, as
 *             nerf_raster_resolve or a renderer's aux maps give them, stacked: images [n, H, W, 3], depth and acc [n, H W];
 *             1 <= H, W <= 16384; near finite and > 0; depth_tol finite and >= 0; cos_min and acc_min in (0, 1].
 *   texel     texel p of the atlas has the position x and the unit normal n of nerf_texture_rows: row[0:3] = x, row[3:6] = -n,
 *             the unclamped extrapolation beyond the hypotenuse and the zero normal included.  A texel of no face, or of a face
 *             with an index outside [0, V), makes no observation and its state is not touched.
 *   camera    `point` of "pinhole camera" at x (zc = 0.0f - z_w); !(zc >= near): no observation (NaN included).  Then (u, v) of
 *             its `pixel`.
 *   facing    e_a = t_a - x_a; L = sqrt((e0 e0 + e1 e1) + e2 e2); cosv = ((n0 e0 + n1 e1) + n2 e2) / L; !(cosv >= cos_min): no
 *             observation.  The weight of the observation is w = cosv.
 *   visible   (i, j) of the camera's `nearest` (floorf(u + 0.5f), floorf(v + 0.5f)); outside the maps: no observation.
 *             a = acc[j W + i], s = depth[j W + i]; a or s NaN, or a < acc_min: no observation.
 *             ez = s / a - zc; !(ez >= 0.0f - depth_tol): no observation, the texel lies behind what the view sees.
 *   colour    a bilinear lookup of the image at (u, v), pixel centres at the integers: x0 = floorf(u), y0 = floorf(v); unless
 *             0 <= x0, x0 + 1 <= W - 1, 0 <= y0 and y0 + 1 <= H - 1, compared as floats: no observation.  fx = u - x0, fy = v - y0,
 *             gx = 1 - fx, gy = 1 - fy; w00 = gx gy, w10 = fx gy, w01 = gx fy, w11 = fx fy (the first index along x, cij the pixel
 *             (x0 + i, y0 + j)); per channel c = ((w00 c00 + w10 c10) + w01 c01) + w11 c11.  A NaN channel: no observation.
 *   state     float32 [W_atlas H_atlas, 4] = (S_c [3], S_w) per texel, 16-byte aligned, zeroed by the caller before the first
 *             view.  NERF_PROJECT_BLEND: S_c = S_c + w c per channel and S_w = S_w + w, in view order.  NERF_PROJECT_BEST: if
 *             w > S_w then S = (c, w); strict, so of equal weights the earlier view stays.
 *   finish    where S_w > 0: c = S_c / S_w (blend) or S_c (best), byte = (uint8)rint(255 unit(c)) as nerf_texture_store; seen = 1.
 *             Elsewhere (NaN included): the byte of `fallback` [H_atlas, W_atlas, 3] uint8 at the texel, 0 without one; seen = 0.
 * Calls:
 *   nerf_project_accumulate  folds views 0 .. n - 1 in order into the state of the texels [p0, p0 + count) of the atlas, one lane
 *                            per texel: the state is loaded once, kept in registers over the views and stored once, which is
 *                            bit-identical to n calls with one view each.  n = 0 or count = 0: nothing is launched.
 *   nerf_project_finish      image [H_atlas, W_atlas, 3] uint8 and seen [H_atlas, W_atlas] uint8 of the same texels; other texels
 *                            are not touched, so neither depends on how the atlas is cut into chunks.
 * The UVs are nerf_texture_uv's.  No atomics, no workspace, no host read; every output element has one writer: bit-reproducible.
 * Out of range: NERF_E_SHAPE; NULL: NERF_E_NULL; all argument checks run before any device work.
 * Not done: no RGBA inputs with alpha-weighted observations, no mipmaps or footprint-sized filtering of the images (one bilinear
 * lookup whatever the texel's size on the screen), no seam levelling between views, no exposure or colour correction between views,
 * no near-plane clipping (the depth maps are the rasteriser's), no inpainting of unseen texels beyond the fallback.             */
#define NERF_PROJECT_MAX_VIEWS 16
#define NERF_PROJECT_BLEND 0
#define NERF_PROJECT_BEST 1
int nerf_project_accumulate(const float* verts, const float* normals, int64_t V, const int32_t* faces, int64_t F, int texels,
                            int64_t p0, int64_t count, const nerf_tsdf_view* views_host, int n, int H, int W, const float* images,
                            const float* depth, const float* acc, float near, float depth_tol, float cos_min, float acc_min, int mode,
                            float* state, void* stream);
int nerf_project_finish(const float* state, int64_t F, int texels, int64_t p0, int64_t count, int mode, const uint8_t* fallback,
                        uint8_t* image, uint8_t* seen, void* stream);

/* ---------------------------------------------------------------- texture mip pyramid (no reference counterpart)
 * Coarser levels for the atlas of "texture atlas", a level of detail per face from its footprint on the screen, and a trilinear
 * lookup through both: a face that covers one pixel is read from the level whose texels are about a pixel wide, not point-sampled
 * from level 0.  The filter is per face, because neighbouring cells of the atlas belong to unrelated faces.  Additive:
 * NERF_ABI_VERSION stays 3.  All float steps are IEEE float32, one rounding per operation (no contraction), in exactly the order
 * and grouping written here; a / b and sqrt are correctly rounded.  csrc/mip.h states the rule in code; tests/_mip_ref.py
 * reproduces every output bit for bit.
 *   levels    T_0 = T; T_{l+1} = (T_l + 1) / 2 in integers while T_l > 2: 8 -> 8, 4, 2; 9 -> 9, 5, 3, 2; 64 -> 64, 32, 16, 8, 4, 2;
 *             2 -> 2.  At most NERF_MIP_MAX_LEVELS.  Level l is a complete atlas of the same F faces: the layout of "texture
 *             atlas" at T_l texels, the UVs of nerf_texture_uv(F, T_l); nerf_texture_sample takes any level unchanged.
 *   reduce    level l (fine: T, S = T + 2) -> level l + 1 (coarse: T', S'), one lane per coarse atlas texel: its face f and local
 *             texel (i, j) by the coarse layout; a texel whose face is >= F is black.  Only the fine image is read, never the mesh.
 *             In-triangle texels, i + j <= T' - 1: x = (float)(i (T - 1)) / (float)(T' - 1), y likewise from j;
 *             r = (float)(T - 1) / (float)(T' - 1), d = 0.25f r; c = lookup(x, y), the bilinear lookup of `sample` in "texture
 *             atlas" at the local texel coordinates (x, y) of face f.  Four antipodal tap pairs (x, y) +- o with the offsets
 *             o = (d, 0), (0, d), (d, d), (d, -d).  A pair counts only if both of its taps (ax, ay) lie in the closed triangle
 *             ax >= 0, ay >= 0, ax + ay <= (float)(T - 1), the sum taken in float32; it then contributes p = lookup(a) + lookup(b),
 *             any other pair p = c + c.  Per channel value = ((p0 + p1) + (p2 + p3)) 0.125f and byte = (uint8)rint(255 unit(value))
 *             as nerf_texture_store.  The centroid of the taps is the texel's own point and every lookup interpolates inside the
 *             face: a constant is kept exactly, an affine field up to rounding, and no read leaves the face's texels.
 *             Gutter texels, the diagonals i + j = T' and then T' + 1, by planar extrapolation of the coarse bytes in integers:
 *             g(i, j) = v(i - 1, j) + v(i, j - 1) - v(i - 1, j - 1) for i, j >= 1; g(i, 0) = 2 v(i - 1, 0) - v(i - 2, 0);
 *             g(0, j) = 2 v(0, j - 1) - v(0, j - 2); clamped to [0, 255]; the second diagonal uses the clamped first.  (Taps that
 *             extrapolate past the hypotenuse instead compound the 8-bit noise from level to level and are not used.)
 *   lod       per face: the snapped face of "mesh rendering" without culling; a dropped face has lod 0.  S = |D| in int64;
 *             g = scale (sqrt((float)S) / 256.0f), the leg in pixels of the right isosceles triangle with the face's screen area;
 *             level l puts T_l - 1 texel steps on it.  lod = 0 with one level or g >= T_0 - 1; lod = L - 1 if g <= T_{L-1} - 1; else
 *             with the l for which T_{l+1} - 1 <= g < T_l - 1: lod = (float)l + ((float)(T_l - 1) - g) / (float)(T_l - T_{l+1}).
 *             Linear in g, no logarithm; isotropic and constant over a face.
 *   sample    lod' = lod clamped to [0, L - 1], NaN -> 0; l = (int)floor(lod'), t = lod' - (float)l; (wb, wc) clamped as `sample`
 *             of "texture atlas"; c_l = lookup on level l at (wb (float)(T_l - 1), wc (float)(T_l - 1)); rgb = c_l when t == 0, else
 *             ((1.0f - t) c_l) + (t c_{l+1}) per channel.  A face outside [0, F) reads black.
 * Calls:
 *   nerf_mip_levels    host only: out = {L, T_0, ..., T_{L-1}, 0 ...}, int32 [1 + NERF_MIP_MAX_LEVELS].  Needs no device.
 *   nerf_mip_reduce    the texels [p0, p0 + count) of the coarse atlas (T' = (texels_fine + 1) / 2) in raster order from the fine
 *                      image; other texels are not touched, a gutter lane recomputes the in-triangle bytes it needs: the image
 *                      depends on neither the chunk nor the launch shape.  texels_fine in [3, 64].
 *   nerf_mip_lod       lod [F] float32 for the camera (a nerf_tsdf_view on the host, "pinhole camera"), near finite and > 0, scale
 *                      finite and > 0, over a pyramid of `texels` at level 0.  One lane per face.  F = 0 launches nothing.
 *   nerf_mip_sample    rgb [n, 3] of n < 2^31 samples face [n] int32, bary [n, 2]; images is a HOST array of the L device
 *                      pointers of the levels of a pyramid over `texels`, handed to the kernel by value; lod is [F] and read at
 *                      the sample's face with per_face = 1, else [n].  n = 0 launches nothing.
 * No atomics, no workspace, no host read; every output element has one writer: bit-reproducible.  Out of range (F or V outside
 * [0, 2^24], texels outside [2, 64], a chunk that leaves the atlas, a scale or near that is not finite and > 0, a non-finite
 * camera): NERF_E_SHAPE; NULL: NERF_E_NULL; all argument checks run before any device work.
 * Not done: no anisotropic or per-pixel footprints (one isotropic lod per face), no filtering of the source pictures in
 * nerf_project_accumulate, no chart packing by area, no seam levelling, no push-pull inpainting of unseen texels over the
 * pyramid, no supersampled coverage, no pyramid inside the OBJ (write_obj writes level 0).                                       */
#define NERF_MIP_MAX_LEVELS 6
int nerf_mip_levels(int texels, int32_t* out_host);
int nerf_mip_reduce(const uint8_t* fine, int64_t F, int texels_fine, uint8_t* coarse, int64_t p0, int64_t count, void* stream);
int nerf_mip_lod(const float* verts, int64_t V, const int32_t* faces, int64_t F, const nerf_tsdf_view* view_host, float near,
                 int texels, float scale, float* lod, void* stream);
int nerf_mip_sample(const uint8_t* const* images_host, int64_t F, int texels, const int32_t* face, const float* bary,
                    const float* lod, int per_face, int64_t n, float* rgb, void* stream);

/* ---------------------------------------------------------------- gradient all-reduce (no reference
 * counterpart: the reference is single-device).  RCCL over xGMI, one in-place float32 sum of the flat gradient
 * buffer per network step.  id: 128 host bytes from nerf_comm_unique_id on rank 0, distributed by the caller.
 * librccl is resolved at first use (NERF_E_RCCL when it is not installed).                                  */
#define NERF_COMM_ID_BYTES 128
int nerf_comm_unique_id(char* id_out_host);
int nerf_comm_init(void** comm_out, int nranks, int rank, const char* id_host);
int nerf_allreduce_grads(void* comm, float* grads, int64_t count, void* stream);
int nerf_comm_destroy(void* comm);

/* runtime selection of kernel variants (for A/B measurement only: none of these changes a result's meaning, a buffer
 * size or a layout; precision is NOT here, it is nerf_mlp_arch.precision):
 *   "mlp_variant"     0 auto | 1,2 weights via L1 (32 / 64 samples per wave) | 3 LDS ring, 32x32x16 MFMA |
 *                     4 LDS ring, 16x16x32 MFMA, 8 waves x 32 samples (render path only; auto picks it there) |
 *                     5 same with 4 waves x 64 samples.  Training kernels use 3 for every value >= 3.
 *   "ring_workgroups" persistent workgroups of the ring kernels (0 = default: one per CU of the current device)
 *   "dw_workgroups"   0 auto (one per CU) | workgroups of the weight-gradient kernel
 *   "dw_unit_bias"    fixed per-tile cost of a dW job, in KiB-of-streaming units, for its static split (negative = automatic, the
 *                     default: 128 for the bf16 kernel, 32 for the split-bf16 kernels)
 *   "dw_private_tiles" split-bf16 weight-gradient jobs of at most this many 32 x 32 output tiles (default 4 = the most; 0 = none) run as
 *                     sixteen independent wave pipelines (no workgroup barrier; fixed-order tree sum at the end) instead of the shared
 *                     4 x 4 wave grid, of which such a job occupies one wave.  Sums in a different order: ~1e-6 rel-L2, bit-reproducible
 *   "dw_ring_cap"     most stages the LDS ring of the 16-wave split-bf16 weight-gradient kernel may hold (default 8; 2 .. 16)
 *   "dw16_variant"    bf16 weight gradients: 1 (default) the 256 x 256 jobs on the one-wave-per-SIMD kernel, job lists of tiny jobs (the
 *                     2 x 64 model) on the split kernels' 16-wave kernel (wave-private pipelines), the other jobs on round 2's 16-wave
 *                     kernel | 0 every job on round 2's kernel | 2, 3: A/B forms of 1 (round 2's / round 5's kernel for every narrow job)
 *   "dw22_variant"    split-bf16 weight gradients: 1 (default) the 256 x 256 jobs on the one-wave-per-SIMD kernel (4 x 4 output tiles
 *                     per wave, two operand register sets), the other jobs on the 16-wave kernel -- two launches | 0 every job on the
 *                     16-wave kernel.  The two sum a tile's products and a bias row in different orders: gradients agree to ~1e-6
 *                     rel-L2, each setting is bit-reproducible from run to run.
 *   "hash_combine_max_res"  table-gradient scatter: levels with N_l <= this value (default 64) accumulate in LDS first and
 *                     add each distinct table entry once (coarse levels collide heavily); 0 = every level directly
 *   "ngp_ray_major"   fused configs[4] inference query: 1 (default) a 32-sample tile is one depth of 32 adjacent rays (the
 *                     lanes of a gather share cells at 13 of 16 levels when rays are neighbouring pixels), 0 = 32
 *                     consecutive depths of one ray.  Same values per sample either way.
 *   "ring_split"      1 (default): one 8-wave workgroup per CU behind a 128 KiB weight ring; 2: two independent 4-wave
 *                     workgroups behind 64 KiB rings (training forward / chain only; measured slower)
 *   "pass_queue"      1 (default): the persistent ring kernels (render forwards, training forwards and chains) hand out their passes
 *                     from a device-wide counter -- a workgroup on a fast XCD takes more passes than one on a slow XCD --; 0: static
 *                     split (pass = blockIdx.x + k gridDim.x).  Bit-identical results: which workgroup runs a pass changes nothing in it.
 *   "f22_tiles"       16-sample tiles per wave of the split-fp16 inference forward on rays + depths (precision 22): 3 (48 samples per
 *                     wave, every weight fragment pair read from the LDS feeds 9 MFMAs) | 2 (rounds 4-5: 32 samples, 6 MFMAs) | 0 (default)
 *                     = 3 except for launches of a few passes per workgroup where whole 32-sample passes divide the work better.  The
 *                     same MFMA sequence per sample: bit-identical results.
 *   "dw_unit_bias"    (see above) automatic = 128 for the bf16 kernels, 2 for the split-bf16 kernels (round 6: was 32)
 *   "dw_narrow_first" order of the two weight-gradient launches: 1 (default) the narrow jobs before the 256 x 256 jobs | 0 after.
 *                     Same gradients either way.
 *   "dw_factor"       weight gradients of the 8 x 256 view model at precision 22: 1 (default) the jobs `feature`, `alpha` and
 *                     `dir0 | feature` run as ONE job (d alpha and dZ_D against H7: G = dZ_D H7^T, db_D) followed by a small post step
 *                     that forms dW_F = W_D[:, :256]^T G, db_F = W_D[:, :256]^T db_D and dW_D[:, :256] = G W_F^T + db_D b_F^T from the
 *                     packed split-bf16 weights in float64 (feature has no activation, so this is exact algebra): H7 is read once
 *                     instead of three times, dZ_F and the stored feature not at all | 0 the three jobs.  G and db_D live in a
 *                     partial-tile slot that is idle at that moment: no workspace size changes.  Other models and precisions, a
 *                     non-zero "dw_job_mask" and "dw22_variant" 0 (one launch over all slots) keep the three jobs whatever this says.
 *                     The affected tensors are summed in a different order (~1e-6 rel-L2); each setting is bit-reproducible.
 *   "train_fold"      split-bf16 TRAINING image and kernels of the 8 x 256 view model at precision 22: 0 (default) the unfolded form |
 *                     1 the feature layer folded into dir0 (W' = W_D[:, :256] W_F, b' = W_D[:, :256] b_F + b_D, each element the float64
 *                     sum in index order rounded once to float32, computed by nerf_mlp_pack): the training forward neither computes
 *                     nor stores `feature`, the chain neither computes nor stores dZ_F (nerf_mlp_debug_read of layer 8 then reads
 *                     whatever the workspace held), and the post step of "dw_factor" takes W_F, W_D[:, :256] and b_F from fp32 copies
 *                     inside the image.  The packed image keeps its size but holds ONE form: nerf_mlp_pack, the training forward and
 *                     nerf_mlp_backward of a model must run under the same setting (models/NeRF.py sets it around its own calls).
 *                     Takes effect only where the factored job list runs ("dw_factor" 1, "dw22_variant" 1, no "dw_job_mask");
 *                     ignored otherwise and by every other model and precision.  sigma is bit-identical to the unfolded form.
 * nerf_get_option returns the current value of EVERY key nerf_set_option accepts (a get / set pair restores a setting;
 * "dw_unit_bias" reads -1 while it is automatic), or NERF_OPTION_UNKNOWN for an unknown key.                        */
#define NERF_OPTION_UNKNOWN (-2147483647 - 1)
int nerf_set_option(const char* key, int value);
int nerf_get_option(const char* key);

/* ---------------------------------------------------------------- optimiser (a21)
 * replaces: mlx.optimizers.Adam.update as called at entrypoints/__test_nerf.py:134,144
 * (mlx 0.7.0: no bias correction unless bias_correction != 0).  g is multiplied by
 * grad_scale first (1/world_size after a sum all-reduce).                               */
int nerf_adam_step(float* params, const float* grads, float* m, float* v, int64_t count, float lr, float beta1,
                   float beta2, float eps, int bias_correction, int step, float grad_scale, void* stream);
/* Same update; grads is float32 [count] (grads_fixed_point = 0) or the int64 [count] fixed-point accumulators of
 * nerf_hashgrid_backward_rays_ex (1), and with zero_grads != 0 the gradient buffer is cleared in the same pass (read g,
 * write 0) so that an accumulating scatter needs no memset before the next step.                                  */
int nerf_adam_step_ex(float* params, void* grads, float* m, float* v, int64_t count, float lr, float beta1, float beta2,
                      float eps, int bias_correction, int step, float grad_scale, int grads_fixed_point, int zero_grads,
                      void* stream);
/* nerf_adam_step_ex that also writes every updated parameter as fp16 to params_half [count] (NULL: exactly
 * nerf_adam_step_ex): the shadow image nerf_ngp_query_fused_h gathers from, kept current at no extra pass.       */
int nerf_adam_step_shadow(float* params, void* grads, float* m, float* v, int64_t count, float lr, float beta1, float beta2,
                          float eps, int bias_correction, int step, float grad_scale, int grads_fixed_point, int zero_grads,
                          void* params_half, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NERF_HIP_H */
