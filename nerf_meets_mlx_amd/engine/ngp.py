"""BASELINE configs[4]: multiresolution hash-grid encoding + tiny fused MLP.

The reference ships the pieces but never wires them (`encoding/multi_hash.py` cannot run, SURVEY Q13;
`encoding/spherical_harmonics.py` has no caller): this module is that wiring, with the reference's own classes --
`MultiHashEncoding(3, 16, 16, 2048, 2, 19)` for positions, `SphericalHarmonicsEncoding(3, 3)` for view directions,
and its `NeRF` class at Instant-NGP size (`NeRF(n_layers=2, width_layers=64, channel_input=32,
channel_input_views=16, list_skip_connection_layers=[], is_use_view_directions=True)`, models/NeRF.py:160-243) --
trained by the coarse-only loop of `render_rays` (rendering/render.py:112-162) + `raw2outputs` + MSE + Adam.

Device work: nerf_hashgrid_forward / nerf_sh_encode -> nerf_mlp_forward_train (2 x 64 kernels) ->
nerf_composite_mse_backward (raw2outputs + MSE + adjoint, one launch) -> nerf_mlp_backward_inputs (dZ chain, dW,
dL/dfeatures) -> nerf_hashgrid_backward_rays_ex per LEVEL GROUP (float atomics, or -- `deterministic=True` -- int64
fixed-point integer atomics whose sum does not depend on the order of the requests) -> nerf_adam_step (MLP) and
nerf_adam_step_ex (tables: reads the accumulated gradient and clears it in the same pass, no memset launch).
With world_size > 1 the table gradient (64 MB float32 / 128 MB int64) is all-reduced group by group on a second
stream while the next group's scatter, the MLP all-reduce and the MLP Adam run (NGPTrainer.train_step).
"""
import ctypes as C
import os
from typing import Dict, Optional

import numpy as np
import torch

from .. import _native as N
from .. import parallel, sampling
from ..encoding.multi_hash import MultiHashEncoding
from ..encoding.spherical_harmonics import SphericalHarmonicsEncoding
from ..models.NeRF import Adam, NeRF, capturing_now
from ..rendering import ray, render
from .trainer import Trainer


class _Flat:
    """Adam-compatible view of a flat trainable buffer (the hash tables)."""

    def __init__(self, params: torch.Tensor, grads: torch.Tensor, half: bool = False):
        self.params, self.grads, self.n_params = params.view(-1), grads.view(-1), params.numel()     # grads: float32 or int64 fixed point
        self.name = "tables"
        # fp16 shadow image of the tables for the forward gathers (4 instead of 8 bytes per entry pair): written by the Adam
        # pass that updates the float32 master (`nerf_adam_step_shadow`), rebuilt from the master whenever somebody else wrote it
        self.half = torch.empty(self.n_params, dtype=torch.float16, device=params.device) if half else None
        self._half_version = -1              # params._version at which the shadow is known to equal fp16(params); -1: stale

    def mark_updated(self, shadow_written: bool = False):
        """Called by Adam after it wrote the master through raw pointers (no torch version bump): with shadow_written it
        wrote EVERY shadow entry in the same pass, so the shadow is current; otherwise it is stale."""
        self._half_version = self.params._version if shadow_written and not capturing_now() else -1     # (a recorded pass wrote nothing yet)

    def shadow(self) -> Optional[torch.Tensor]:
        """The fp16 image, current with the float32 master (None when the model was built without one).  Rebuilt by one
        conversion pass after construction, load_flat, or a torch in-place edit of the tables (version counter).  Under stream
        capture the conversion is always enqueued -- the graph carries its own -- and the shadow keeps counting as stale, since
        a recorded conversion has not run (DESIGN.md "Graph capture").  (Replays need no flag here: the Adam pass that writes
        the master, recorded or not, writes every shadow entry with it.)"""
        if self.half is None:
            return None
        if capturing_now():
            self.half.copy_(self.params)
            self._half_version = -1
        elif self._half_version != self.params._version:
            self.half.copy_(self.params)
            self._half_version = self.params._version
        return self.half

    def load_flat(self, flat: torch.Tensor):
        assert flat.numel() == self.n_params
        with torch.no_grad():
            self.params.copy_(flat.to(self.params.device, torch.float32).reshape(-1))
        self._half_version = -1


class HashNeRF:
    """positions -> hash grid (32) | view directions -> SH degree 3 (16) -> NeRF 2 x 64 -> raw [rgb, sigma]."""

    def __init__(self, device="cuda", seed: int = 0, n_levels: int = 16, min_res: int = 16, max_res: int = 2048,
                 n_features_per_level: int = 2, log2_hashmap_size: int = 19, hash_init_scale: float = 1e-4,
                 bound: Optional[float] = 1.5, deterministic: bool = True, level_groups: int = 4,
                 half_tables: Optional[bool] = None, precision: int = 22):
        """precision: arithmetic of the 2 x 64 network (`NeRF(precision=...)`).  22 (default): the reference's float32 tolerance
        -- float32 gathers from the master tables, float32 interpolation (encoding/multi_hash.py:112-131), split-bf16 MLP
        (csrc/mlp_s16x.hip); 16: the declared reduced-precision mode (bf16 MLP operands, interpolated features rounded to bf16).
        half_tables (precision 16 only; default on there): the fused query gathers from an fp16 shadow image of the tables (half
        the gather bytes; float32 master, float32 interpolation; the bf16 MLP rounds the interpolated features to 8 bits anyway)
        -- SURVEY 8(d)'s 512 B per sample.  Refused at precision 22, whose point is not to round the features.
        bound: half-extent of the scene box that is mapped onto the grid's unit cube before hashing
        (x' = (x + bound) / (2 bound)), so that N_l is the level's resolution ACROSS the scene (without it the reference's
        x * N_l sees world units: 3 x finer cells, and a 24-view run memorises its training rays: held-out PSNR 13.8 dB
        at a training loss of 1e-3).  None = world coordinates, the bare reference formula."""
        assert n_levels * n_features_per_level == 32, "the 2 x 64 kernels take 32 position features"
        self.enc = MultiHashEncoding(3, n_levels, min_res, max_res, n_features_per_level, log2_hashmap_size,
                                     hash_init_scale, device=device, seed=seed)
        self.sh = SphericalHarmonicsEncoding(3, 3)
        self.mlp = NeRF(n_layers=2, width_layers=64, channel_input=32, channel_input_views=16,
                        list_skip_connection_layers=[], is_use_view_directions=True, device=device, seed=seed, precision=precision)
        self.precision = int(precision)
        if half_tables is None:
            half_tables = self.precision == 16
        if half_tables and self.precision != 16:
            raise ValueError("HashNeRF: half_tables (fp16 shadow gathers) is a reduced-precision option of precision=16")
        self.bound = bound
        self.pos_scale, self.pos_offset = (1.0, 0.0) if bound is None else (1.0 / (2.0 * bound), 0.5)
        # table-gradient accumulator: int64 2^-52 fixed point added with integer atomics (the default: bit-reproducible, and
        # measured no slower than float atomics -- both are bound by the atomic request rate, profiles/r03_ngp_scatter.csv)
        # or float32 (float atomics, order-dependent rounding).  The Adam pass that consumes it clears it: no memset.
        self.deterministic = bool(deterministic)
        if self.deterministic:
            self.enc.grad = torch.zeros(self.enc.tables.shape, dtype=torch.int64, device=self.enc.tables.device)
        self.table = _Flat(self.enc.tables, self.enc.grad, half=bool(half_tables) and n_features_per_level == 2)
        # True while the accumulator is known to hold zeros (fresh, or consumed-and-cleared by nerf_adam_step_ex); any
        # scatter makes it dirty.  NGPTrainer.train_step only skips the clear when this says so: a public backward() call,
        # or a step that raised between the scatter and Adam, leaves a gradient behind that must not be added to the next one.
        self._grad_clean = True
        ng = max(1, min(int(level_groups), n_levels))
        self.level_groups = [(n_levels * i // ng, n_levels * (i + 1) // ng) for i in range(ng)]
        self.on_group_done = None           # NGPTrainer: called after each level group's scatter is enqueued (lo, hi)
        self.on_mlp_grads = None            # NGPTrainer: called with the MLP gradient as soon as it is enqueued (before the scatters)
        self._pts, self._rz = None, None
        self._sel = None                    # culled training query: (kept sample indices [K], B, n); None: every sample ran
        self.fused = os.environ.get("NERF_NGP_FUSED", "1") != "0"      # rows inside the forward kernel (default) or through HBM
        self.timing = None                  # bench.py: list that receives (start, end) events around the table scatter
        self._bwd_lw = None                 # level weights captured by the last query(train=True): backward() uses these

    @property
    def level_weights(self):
        """Per-level weights of the hash encoding (a tuple of n_levels numbers in [0, 1]) or None, the default: every path then
        passes NULL weights and runs the same kernels as without the option.  features, features_unfused, query (fused, unfused,
        culled, packed) and backward use them; backward uses the weights captured by the last query(train=True), not the current
        property."""
        return self.enc.level_weights

    @level_weights.setter
    def level_weights(self, w):
        self.enc.level_weights = w

    def features(self, rays: torch.Tensor, z: torch.Tensor, need_pts: bool = True):
        """x [B n, 48] = [MultiHashEncoding(o + z d) | SphericalHarmonicsEncoding(viewdirs)] in one call
        (`nerf_ngp_encode`), and the sample positions for the table-gradient pass."""
        B, n = z.shape
        e = self.enc
        x = torch.empty(B * n, 48, dtype=torch.float32, device=z.device)
        pts = torch.empty(B * n, 3, dtype=torch.float32, device=z.device) if need_pts else None
        N.check(N.lib().nerf_ngp_encode_lw(N.ptr(N.f32(rays)), N.ptr(N.f32(z)), B, n, N.ptr(e.tables), e.n_levels,
                                           e.log2_hashmap_size, e.n_features_per_level, e._res_c, e._lw_c, 3, self.pos_scale,
                                           self.pos_offset, N.ptr(x), N.ptr(pts), N.stream()))
        return pts, x

    def features_unfused(self, rays: torch.Tensor, z: torch.Tensor):
        """The same rows from the stand-alone encoder classes (tests compare the two)."""
        B, n = z.shape
        pts = (rays[:, None, 0:3] + z[:, :, None] * rays[:, None, 3:6]).reshape(-1, 3)     # render.py:142
        pts = pts * self.pos_scale + self.pos_offset                                       # scene box -> unit cube
        feat = self.enc(pts)                                                               # [B n, 32]
        shf = self.sh(rays[:, 8:11].contiguous())                                          # [B, 16]
        x = torch.cat([feat.view(B, n, 32), shf[:, None, :].expand(B, n, 16)], dim=-1).reshape(B * n, 48)
        return pts, x

    def query(self, rays: torch.Tensor, z: torch.Tensor, train: bool = False, fused: Optional[bool] = None,
              grid=None) -> torch.Tensor:
        """raw [B,n,4].  fused (default): hash gathers and SH are evaluated inside the 2 x 64 forward kernel
        (`nerf_ngp_query_fused`), no [B n, 48] rows in HBM; fused=False goes through `features` + `mlp.forward`.
        grid (an engine.occupancy.OccupancyGrid): only the samples in occupied cells are evaluated (fused query on the K kept
        rows, one host read of K); the others get raw (0, 0, 0, 0).  With train=True, backward() follows the kept samples."""
        B, n = z.shape
        if fused is None:
            fused = self.fused
        if grid is not None:
            if not fused:
                raise ValueError("HashNeRF.query: the occupancy-grid path runs on the fused query (fused=False has no culled form)")
            if self.bound is None:
                raise ValueError("HashNeRF.query: an occupancy grid needs a scene box (HashNeRF(bound=None) has none)")
            return self._query_culled(rays, z, train, grid)
        if train:
            self._sel = None
            self._bwd_lw = self.enc._lw_c
        if not fused:
            pts, x = self.features(rays, z, need_pts=train)
            self._pts, self._rz = (pts if train else None), None
            return self.mlp.forward(x, train=train).view(B, n, 4)
        e, m = self.enc, self.mlp
        rays, z = N.f32(rays), N.f32(z)
        raw = torch.empty(B, n, 4, dtype=torch.float32, device=z.device)
        acts = None
        if train:
            acts = m._begin_train_pass(B * n)
            self._pts, self._rz = None, (rays, z)
        N.check(N.lib().nerf_ngp_query_fused_lw(C.byref(m.arch), N.ptr(m.packed()), N.ptr(rays), N.ptr(z), B, n,
                                                N.ptr(e.tables), N.ptr(self.table.shadow()), e.n_levels, e.log2_hashmap_size,
                                                e.n_features_per_level, e._res_c, e._lw_c, 3, self.pos_scale,
                                                self.pos_offset, N.ptr(raw), N.ptr(acts), N.stream()))
        return raw

    def _query_culled(self, rays, z, train, grid):
        from .occupancy import scatter_rows
        B, n = z.shape
        idx, rk, zk, raw, K = grid.cull(rays, z)
        if K > 0:
            raw_k = self.query(rk, zk, train=train)             # B = K, n = 1: the unchanged fused query (sets _rz when training)
            if grid.timing is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            scatter_rows(raw_k, idx, raw)
            if grid.timing is not None:
                e1.record()
                grid.timing.append(("scatter", e0, e1))
        elif train:
            self._rz, self._pts = None, None
            self._bwd_lw = self.enc._lw_c
        if train:
            self._sel = (idx, B, n)
        return raw

    def query_packed(self, rows: torch.Tensor, z: torch.Tensor, train: bool = False) -> torch.Tensor:
        """raw [K, 1, 4] of K packed samples (rows [K, 11], depths z [K]: the output of OccupancyGrid.march) as one B = K, n = 1
        fused query.  K = 0 is allowed: with train=True, backward() then gives a zero MLP gradient and still runs every
        level-group hook."""
        K = rows.shape[0]
        if K > 0:
            return self.query(rows, z.reshape(K, 1), train=train, fused=True)
        if train:
            self._sel = (torch.empty(0, dtype=torch.int64, device=rows.device), 0, 1)
            self._rz, self._pts = None, None
            self._bwd_lw = self.enc._lw_c
        return torch.empty(0, 1, 4, dtype=torch.float32, device=rows.device)

    def table_grad(self) -> torch.Tensor:
        """The accumulated table gradient as float32 [L,T,F] (a copy when the accumulators are int64 fixed point)."""
        g = self.enc.grad
        return (g.double() * 2.0 ** -52).float() if g.dtype == torch.int64 else g

    def backward(self, d_raw: torch.Tensor, accumulate: bool = False):
        """(MLP gradient [13188], table gradient [L,T,F]: float32, or int64 2^-52 fixed point when deterministic) of the
        last query(train=True).  accumulate=True adds into the gradient buffer as it stands (NGPTrainer: the Adam pass that
        consumed the previous gradient left it zeroed); the default clears it first."""
        K = None
        if self._sel is not None:                            # culled query: the gradient of the kept samples' raw rows only
            from .occupancy import gather_rows
            idx, B, n = self._sel
            assert d_raw.numel() == B * n * 4, "backward() needs the d_raw of the last query(train=True)"
            K = idx.numel()
            d_raw = gather_rows(d_raw.reshape(B * n, 4), idx)
        if K == 0:                                           # nothing was evaluated: zero MLP gradient, no scatter
            grads, d_x = self.mlp.grads, None
            grads.zero_()
        else:
            grads, d_x = self.mlp.backward(d_raw, need_input_grad=True)
        if self.on_mlp_grads is not None:
            self.on_mlp_grads(grads)
        e = self.enc
        if not accumulate:
            e.grad.zero_()
        self._grad_clean = False
        if self.timing is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        if K == 0:
            for lo, hi in self.level_groups:                 # the multi-rank hooks still run: every rank joins every collective
                if self.on_group_done is not None:
                    self.on_group_done(lo, hi)
        elif self._rz is None:                               # unfused rows: positions were kept by features()
            e.backward(self._pts, d_x, level_weights=self._bwd_lw)
            if self.on_group_done is not None:
                self.on_group_done(0, e.n_levels)
        else:
            rays, z = self._rz
            for lo, hi in self.level_groups:
                N.check(N.lib().nerf_hashgrid_backward_rays_ex_lw(       # the weights of the forward pass this is the gradient of
                    N.ptr(rays), N.ptr(z), z.shape[0], z.shape[1], N.ptr(d_x), e.n_levels, e.log2_hashmap_size,
                    e.n_features_per_level, e._res_c, self._bwd_lw, self.pos_scale, self.pos_offset, lo, hi,
                    int(self.deterministic), N.ptr(e.grad), N.stream()))
                if self.on_group_done is not None:
                    self.on_group_done(lo, hi)
        if self.timing is not None:
            e1.record()
            self.timing.append((e0, e1))
        return grads, e.grad


def check_level_anneal(level_anneal, n_levels: int):
    """None or (start_levels, iters): integers with 1 <= start_levels <= n_levels and iters >= 1, else ValueError."""
    if level_anneal is None:
        return None
    try:
        start, iters = level_anneal
    except (TypeError, ValueError):
        raise ValueError(f"level_anneal must be None or (start_levels, iters), got {level_anneal!r}") from None
    for name, v in (("start_levels", start), ("iters", iters)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"level_anneal: {name} must be an integer, got {v!r}")
    if not 1 <= start <= n_levels:
        raise ValueError(f"level_anneal: need 1 <= start_levels <= {n_levels}, got {start}")
    if iters < 1:
        raise ValueError(f"level_anneal: need iters >= 1, got {iters}")
    return int(start), int(iters)


def level_anneal_from_text(text: str):
    """'START,ITERS' (the --level-anneal flag of the tools) -> (start_levels, iters); ValueError for anything else."""
    try:
        start, iters = (int(v) for v in text.split(","))
    except (AttributeError, ValueError):
        raise ValueError(f"level_anneal: need START,ITERS (two integers), got {text!r}") from None
    return start, iters


def level_anneal_weights(start_levels: int, iters: int, n_levels: int, it: int):
    """w_l = min(1, max(0, alpha - l)), alpha = start_levels + (L - start_levels) min(1, it / iters), in double on the host,
    rounded to float32 (returned as Python floats)."""
    import numpy as np
    alpha = float(start_levels) + float(n_levels - start_levels) * min(1.0, float(it) / float(iters))
    return tuple(float(np.float32(min(1.0, max(0.0, alpha - l)))) for l in range(n_levels))


def _cat(outs, aux: bool):
    """torch.cat of the per-chunk outputs of render_rays (dicts of tensors when aux)."""
    if not aux:
        return torch.cat(outs, 0)
    return {k: torch.cat([o[k] for o in outs], 0) for k in outs[0]}


class NGPTrainer(Trainer):
    """Coarse-only training / rendering loop on a HashNeRF (one network, `n_depth_samples` stratified-grid samples per
    ray, no importance pass).  Rays shard across ranks; MLP and table gradients are sum-all-reduced before Adam."""

    def __init__(self, images, poses, K, near: float = 2.0, far: float = 6.0, N_rand: int = 4096,
                 n_depth_samples: int = 64, lrate: float = 5e-4, lrate_decay: int = 500, white_bkgd: bool = True,
                 seed: int = 0, device="cuda", chunk: int = 1024 * 32, table_sync: str = "shard", precision: int = 22,
                 occupancy_grid: bool = False, march_steps: Optional[int] = None, min_transmittance: Optional[float] = None,
                 distortion_weight: Optional[float] = None, random_background: bool = False, level_anneal=None, **hash_kw):
        """occupancy_grid: empty-space skipping (engine/occupancy.py): the grid is updated every UPDATE_EVERY iterations from the
        start; from iteration WARMUP on, training and rendering evaluate only the samples in occupied cells.  Off by default.
        march_steps (needs occupancy_grid=True and a scene box; 1 ... 1024; None: the n_depth_samples stratified grid): the
        occupancy-guided ray march of DESIGN.md section 12 replaces the fixed samples -- each ray is stepped at
        sqrt(3) / march_steps * 2 bound through the box, only the steps in occupied cells (every step inside the box before
        WARMUP) are evaluated, and they are composited with sigma = trunc_exp(raw).
        random_background (needs march_steps and images [N, H, W, 4], straight RGBA in [0, 1] as load_blender_data returns them;
        DESIGN.md section 16): every training ray gets a colour bg uniform in [0, 1)^3 (counter stream 5), the target is
        rgb_gt a_gt + bg (1 - a_gt) and the rendered ray sum w c + (1 - acc) bg, so that opacity is supervised.  A constructor
        setting like distortion_weight: not checkpointed.  Off by default.
        level_anneal = (start_levels, iters) (any mode, any precision): a coarse-to-fine schedule over the
        hash levels.  At iteration `it` level l has the weight w_l = clamp(alpha - l, 0, 1) with alpha = start_levels +
        (L - start_levels) min(1, it / iters) (`level_weights_at`): train_step sets the field's level_weights from self.it
        before the forward pass, rendering uses the weights of the current `it`, and from it >= iters on the weights are None
        again (the kernels without the option).  While it is set the trainer owns field.level_weights and overwrites a value
        assigned by hand.  A constructor setting, not checkpointed: after load the weights follow from the restored `it`.  Off
        by default."""
        self._n_levels = int(hash_kw.get("n_levels", 16))
        self.level_anneal = check_level_anneal(level_anneal, self._n_levels)
        if march_steps is not None:
            from .occupancy import check_march_steps
            check_march_steps(march_steps)
            if not occupancy_grid:
                raise ValueError("NGPTrainer: march_steps needs occupancy_grid=True (the march samples the grid)")
            if hash_kw.get("bound", 1.5) is None:
                raise ValueError("NGPTrainer: march_steps needs a scene box (HashNeRF(bound=None) has none)")
        if min_transmittance is not None:
            from .occupancy import check_min_transmittance
            min_transmittance = check_min_transmittance(min_transmittance)
            if march_steps is None:
                raise ValueError("NGPTrainer: min_transmittance needs march_steps (early termination is a mode of the march)")
        if distortion_weight is not None:
            from .occupancy import check_distortion_weight
            distortion_weight = check_distortion_weight(distortion_weight)
            if march_steps is None:
                raise ValueError("NGPTrainer: distortion_weight needs march_steps (the regulariser acts on the march's packed samples)")
        channels = None if images is None else int(images.shape[-1])
        if random_background:
            if march_steps is None:
                raise ValueError("NGPTrainer: random_background needs march_steps (the background is a mode of the march's packed "
                                 "compositing)")
            if channels != 4:
                raise ValueError(f"NGPTrainer: random_background needs RGBA images [N, H, W, 4], got {channels} channels")
        elif channels == 4:
            raise ValueError("NGPTrainer: images with 4 channels (RGBA) need random_background=True (and march_steps); fold them "
                             "onto a background first otherwise, e.g. with dataset.dataloader.post_load_blender_data")
        self.random_background = bool(random_background)
        self.march_steps = march_steps
        self.min_transmittance = min_transmittance
        self.distortion_weight = distortion_weight
        super().__init__(images, poses, K, near=near, far=far, N_rand=N_rand, n_depth_samples=n_depth_samples,
                         N_importance=0, lrate=lrate, lrate_decay=lrate_decay, white_bkgd=white_bkgd, ref_quirks=True,
                         seed=seed, device=device, chunk=chunk, precision=precision)
        self.coarse = None                                   # the 8 x 256 network of the base class is not used
        self._field = HashNeRF(device=self.device, seed=seed, precision=precision, **hash_kw)
        self._field.mlp.name = "mlp"
        self._apply_level_weights()
        self.grid = None
        self.last_march = None               # march mode: (rays, kept samples) of the last training march
        if occupancy_grid:
            from .occupancy import OccupancyGrid
            self.grid = OccupancyGrid(self._field, near, far, n_depth_samples, seed=seed, device=self.device,
                                      march_steps=march_steps)
        self._march_gen = torch.Generator(device=self.device) if march_steps is not None else None
        self._bg_gen = torch.Generator(device=self.device) if self.random_background else None
        # Adam WITH bias correction: without it the first steps are lr * sign(g), which turns bf16 noise in near-zero
        # table gradients into full-size steps and can drive sigma negative everywhere (a dead network under the
        # reference's un-activated sigma).  This loop is our wiring, so the choice is ours; lrate is
        # the reference's 5e-4 (at 2e-3 both this trainer and the fp32 oracle collapse to sigma < 0 within 200 iterations).
        self.opt = Adam(lrate, betas=(0.9, 0.99), eps=1e-8, bias_correction=True, shared_state=False)
        self._comm = torch.cuda.Stream(device=self.device) if self.world > 1 else None
        # How the table gradient is combined across ranks (world_size > 1):
        #   "allreduce": every level group's accumulator slice is sum-all-reduced, every rank steps all 16.8 M entries
        #                (int64 accumulators: 134 MB on the wire twice per step);
        #   "shard"    : reduce-scatter of the accumulators (each rank receives the sum of ITS 1/W of every level group), Adam on
        #                the owned shards only, all-gather of the updated float32 tables: 134 (W-1)/W + 67 (W-1)/W MB instead of
        #                2 x 134 (W-1)/W, a W-th of the Adam work, and exact integer sums as before (bit-identical tables on all
        #                ranks, run to run, and identical to the all-reduce schedule).  Adam moments are sharded with the
        #                parameters: `sync_optimizer_state()` gathers them -- an explicit COLLECTIVE every rank calls at the same
        #                iteration; state_dict() / save() never communicate and RAISE while the moments are stale, so the
        #                usual "if rank == 0: save()" idiom cannot hang in a collective the other ranks never enter.
        if table_sync not in ("shard", "allreduce"):
            raise ValueError("NGPTrainer: table_sync must be 'shard' or 'allreduce'")
        per_group = [(hi - lo) * self._field.enc.hash_table_size * self._field.enc.n_features_per_level for lo, hi in self._field.level_groups]
        self.table_sync = table_sync if (self.world > 1 and all(n % self.world == 0 for n in per_group)) else "allreduce"
        self._rs_bufs = None
        self._moments_synced = True          # no step taken yet: nothing sharded

    # `field` (tables, MLP) may still be receiving the other ranks' updated shards on the comm stream when train_step returns:
    # reading it from outside joins that stream first (a stream-side wait, no host block).  The hot loop uses _field.
    @property
    def field(self):
        self._join_comm()
        return self._field

    @field.setter
    def field(self, f):
        self._field = f

    def level_weights_at(self, it: int):
        """The level weights at iteration `it`: None without level_anneal and from it >= iters on (every weight is exactly 1
        then), else a tuple of n_levels float32-rounded numbers (`level_anneal_weights`)."""
        if self.level_anneal is None or it >= self.level_anneal[1]:
            return None
        return level_anneal_weights(self.level_anneal[0], self.level_anneal[1], self._n_levels, it)

    def _apply_level_weights(self):
        """Sets the field's weights from self.it (identical on every rank: they depend on `it` only).  Called wherever `it`
        changes -- the constructor, the end of train_step, load_state_dict -- so rendering, the distortion loss and mesh export
        find the field current, and once more at the top of train_step, which DESIGN.md section 19 promises.  With level_anneal
        set the trainer owns the field's level_weights: a value assigned to field.level_weights by hand is overwritten here."""
        if self.level_anneal is not None:
            self._field.level_weights = self.level_weights_at(self.it)

    def _mesh_field(self):
        """The hash-grid field through `field` (joins the comm stream); exp density in march mode, relu otherwise."""
        from .mesh import EXP, RELU
        f = self.field
        return (lambda rays, z: f.query(rays, z)), (EXP if self.march_steps is not None else RELU)

    def _mesh_box(self, aabb):
        """aabb, or the field's scene box [-bound, bound]^3 by default."""
        if aabb is not None:
            return super()._mesh_box(aabb)
        b = self._field.bound
        if b is None:
            raise ValueError("NGPTrainer mesh export: the field has no scene box (bound=None), pass aabb=(lo, hi)")
        return [-float(b)] * 3, [float(b)] * 3

    def render_depth(self, c2w):
        """(depth [H, W], acc [H, W]) of the full frame at pose c2w: the "depth" (sum w z, not normalised; depth / acc is distance
        along the optical axis) and "acc" of render_rays(aux=True), in every hash-grid mode.  This rank only, no collective."""
        c = np.asarray(c2w.detach().cpu().numpy() if torch.is_tensor(c2w) else c2w)[:3, :4]
        idx = torch.arange(0, self.H * self.W, device=self.device, dtype=torch.int64)
        rays = ray.gen_rays(self.H, self.W, self.K, c, self.near, self.far, idx)
        o = self.render_rays(rays, aux=True)
        return o["depth"].reshape(self.H, self.W), o["acc"].reshape(self.H, self.W)

    def mesh_depth_error(self, mesh, c2w, acc_min: float = 0.5, resolution: int = 256, aabb=None) -> dict:
        """A mesh against the field it came from, ray for ray over the frame at pose c2w: engine.mesh.raycast_frame along the rays
        render_depth renders (near, far, K as the trainer's) against render_depth's depth / acc where acc >= `acc_min`.  Returns
        {"mean", "rms"}: the mean and root-mean-square |mesh depth - field depth| over the pixels where both see a surface, in
        units of h = the longest side of the scene box (`aabb` as in extract_mesh) / `resolution`, NaN when there is no such
        pixel; {"both", "mesh_only", "field_only", "neither"}: the shares of the frame's pixels, which sum to 1; and "h".
        This rank only, no collective."""
        from . import mesh as M
        lo, hi = self._mesh_box(aabb)
        R = M.check_mesh_args(resolution, lo, hi)[0]
        if not isinstance(acc_min, (int, float)) or isinstance(acc_min, bool) or not 0.0 < float(acc_min) <= 1.0:
            raise ValueError(f"mesh_depth_error: acc_min must be a number in (0, 1], got {acc_min!r}")
        h = max(b - a for a, b in zip(lo, hi)) / R
        _, _, m_depth, m_acc, _ = M.raycast_frame(mesh, c2w, self.K, self.H, self.W, near=float(self.near), far=float(self.far))
        f_depth, f_acc = self.render_depth(c2w)
        seen_m, seen_f = m_acc > 0, f_acc >= float(acc_min)
        both = seen_m & seen_f
        n, nb = float(seen_m.numel()), int(both.sum())
        diff = (m_depth.double() - f_depth.double() / f_acc.double().clamp_min(1e-12))[both].abs() / h
        return {"mean": float(diff.mean()) if nb else float("nan"), "rms": float(diff.pow(2).mean().sqrt()) if nb else float("nan"),
                "both": nb / n, "mesh_only": int((seen_m & ~seen_f).sum()) / n, "field_only": int((~seen_m & seen_f).sum()) / n,
                "neither": int((~seen_m & ~seen_f).sum()) / n, "h": h}

    def extract_mesh_tsdf(self, resolution: int = 256, aabb=None, poses=None, trunc=None, acc_min: float = 0.5, carve: bool = True,
                          min_views: int = 1, colors: bool = True, min_component: int = 0, largest_only: bool = False,
                          opening_radius: int = 0, simplify_grid: int = 0, simplify_placement: str = "quadric",
                          smooth_iterations: int = 0, smooth_lambda: float = 0.5, smooth_mu: float = -0.53):
        """engine.mesh.Mesh of the zero level set of a TSDF fused from this field's own depth renders (DESIGN.md section 21;
        KinectFusion, nerfstudio's TSDF export): render_depth at every pose of `poses` ([n, 3 or 4, 4]; None: the training
        poses), engine.mesh.TSDFVolume(resolution, box, trunc).integrate with far = the trainer's far, volume(min_views), the
        component filter or the opening of extract_mesh at iso 0, marching cubes at 0, and vertex colours (when `colors`) from
        the field queried at each vertex along -normal.  A voxel is inside only if the cameras agree a surface lies in front of
        it; a ray with opacity below `acc_min` carves (with `carve`) every voxel along it.  trunc=None: 4 voxels
        (TSDFVolume).  The order of `poses` is the fusion order and fixes the bits of the result: the running mean is a
        float32 recurrence, so another order may differ in the last place.  `simplify_grid` / `simplify_placement` as in
        extract_mesh: the mesh is clustered before it is coloured; `smooth_iterations` / `smooth_lambda` / `smooth_mu` as in
        extract_mesh: the mesh is smoothed before it is clustered.  Runs on this rank only, no collective."""
        from . import mesh
        lo, hi = self._mesh_box(aabb)
        R = mesh.check_mesh_args(resolution, lo, hi, 0.0)[0]
        volume_options = mesh.check_volume_options(min_component, largest_only, opening_radius, R)
        mesh.check_tsdf_args(trunc, acc_min, self.far, carve, min_views, self.H, self.W)
        surface_options = mesh.check_surface_options(simplify_grid, simplify_placement, smooth_iterations, smooth_lambda, smooth_mu)
        poses = self.poses if poses is None else poses
        views = mesh.tsdf_views(poses, self.K)
        tsdf = mesh.TSDFVolume(R, lo, hi, trunc=trunc, device=self.device)
        c2ws = views[:, :12].reshape(-1, 3, 4)
        for s in range(0, len(c2ws), mesh.TSDF_MAX_VIEWS):
            batch = c2ws[s:s + mesh.TSDF_MAX_VIEWS]
            maps = [self.render_depth(c) for c in batch]
            tsdf.integrate(torch.stack([m[0] for m in maps]), torch.stack([m[1] for m in maps]), batch, self.K, self.H, self.W,
                           acc_min=acc_min, far=self.far, carve=carve)
        vol = tsdf.volume(min_views)
        del tsdf
        vol = mesh.filter_volume(vol, 0.0, *volume_options)
        query = self._mesh_field()[0] if colors else None          # (reading the field joins the comm stream: only when it is asked)
        return mesh.mesh_volume(query, vol, 0.0, lo, hi, colors, *surface_options)

    def train_step(self, rays=None, target=None, u=None, background=None) -> Dict[str, torch.Tensor]:
        """background (random_background trainers only, with explicit rays and target [B, 4]): the colours bg [B, 3] behind the
        rays instead of the ones drawn from counter stream 5."""
        if background is not None and not self.random_background:
            raise ValueError("NGPTrainer.train_step: background needs a trainer built with random_background=True")
        if rays is None:
            rays, target = self.sample_batch()
        self._apply_level_weights()
        self._opt.learning_rate = self.lrate * (0.1 ** (self.it / (self.lrate_decay * 1000)))
        if self.march_steps is not None:
            self._join_comm()
            loss, d_raw, dist = self._march_step_forward(rays, target, background)
        else:
            z = sampling.sample_coarse(rays, self.n)
            self._join_comm()                                # the previous step's table all-gathers (sharded updates)
            raw = self._field.query(rays, z, train=True, grid=self._grid_for_step(update=True))
            loss, d_raw, _ = render.composite_mse_backward(raw, z, rays, target, self.white_bkgd)
        pending, mlp_work = [], []
        shard = self.world > 1 and self.table_sync == "shard"
        if self.world > 1:
            # Collectives of one process group run in issue order, so the small MLP gradient goes FIRST (it is complete
            # before the scatters start), then each level group's slice of the table gradient as soon as its scatter is
            # enqueued -- all on the comm stream, behind events: the transfers overlap the following groups' scatters,
            # and the MLP Adam runs while the table slices are still on the wire.
            per_level = self._field.enc.hash_table_size * self._field.enc.n_features_per_level
            flat = self._field.table.grads

            def on_comm(t):
                ev = torch.cuda.Event()
                ev.record()
                self._comm.wait_event(ev)
                with torch.cuda.stream(self._comm):
                    return torch.distributed.all_reduce(t, async_op=True)
            self._field.on_mlp_grads = lambda g: mlp_work.append(on_comm(g))
            if shard:
                if self._rs_bufs is None or self._rs_bufs[0].dtype != flat.dtype:
                    self._rs_bufs = [torch.empty((hi - lo) * per_level // self.world, dtype=flat.dtype, device=flat.device)
                                     for lo, hi in self._field.level_groups]

                def on_group(lo, hi):
                    gi = self._field.level_groups.index((lo, hi))
                    ev = torch.cuda.Event()
                    ev.record()
                    self._comm.wait_event(ev)
                    with torch.cuda.stream(self._comm):
                        pending.append(torch.distributed.reduce_scatter_tensor(self._rs_bufs[gi], flat[lo * per_level:hi * per_level],
                                                                               async_op=True))
                self._field.on_group_done = on_group
            else:
                self._field.on_group_done = lambda lo, hi: pending.append(on_comm(flat[lo * per_level:hi * per_level]))
        # accumulate (no clear) only when the accumulator is KNOWN to be zero: left so by the previous step's table Adam
        g_mlp, g_tab = self._field.backward(d_raw, accumulate=self._field._grad_clean)
        self._field.on_group_done = self._field.on_mlp_grads = None
        for w in mlp_work:
            w.wait()
        self._opt.update(self._field.mlp, g_mlp, grad_scale=1.0 / self.world)      # _opt: the `opt` property would join the comm stream
        for w in pending:
            w.wait()
        if pending:
            torch.cuda.current_stream().wait_stream(self._comm)
        if shard:
            # Adam on the owned 1/W of every level group (sums received by the reduce-scatter), then every rank gets the others'
            # updated entries; the accumulator was consumed by the collectives: clear it (one 134 MB memset, ~30 us)
            params = self._field.table.params
            spans = []
            for (lo, hi), buf in zip(self._field.level_groups, self._rs_bufs):
                n = buf.numel()
                spans.append((lo * per_level + self.rank * n, lo * per_level + (self.rank + 1) * n, buf))
            self._opt.update_spans(self._field.table, spans, grad_scale=1.0 / self.world)
            self._moments_synced = False
            flat.zero_()
            # all-gathers of the updated shards on the comm stream, one per level group, behind the Adam launches; the next
            # step's forward (the first reader of the tables) joins that stream
            half = self._field.table.half
            ev = torch.cuda.Event()
            ev.record()
            self._comm.wait_event(ev)
            with torch.cuda.stream(self._comm):
                for (lo, hi), (a, b, _) in zip(self._field.level_groups, spans):
                    torch.distributed.all_gather_into_tensor(params[lo * per_level:hi * per_level], params[a:b].clone())
                    if half is not None:     # the fp16 shadow shards Adam wrote in the same pass travel too: no re-conversion
                        torch.distributed.all_gather_into_tensor(half[lo * per_level:hi * per_level], half[a:b].clone())
            if half is not None:
                self._field.table.mark_updated(shadow_written=True)
        else:
            self._opt.update(self._field.table, g_tab.view(-1), grad_scale=1.0 / self.world, zero_grads=True)    # reads g, writes 0
        self._field._grad_clean = True
        self.it += 1
        self._apply_level_weights()                          # rendering sees the weights of the current iteration
        if self.distortion_weight is not None:
            return {"loss_coarse": loss, "loss_distortion": dist}
        return {"loss_coarse": loss}

    def _march_step_forward(self, rays, target, background=None):
        """March mode, training: grid update -> march (per-ray jitter from counter stream 4) -> fused query of the K packed
        samples -> packed compositing + MSE backward, with the distortion regulariser when distortion_weight is set and over a
        random background per ray (counter stream 5, unless `background` [B, 3] is given) against the RGBA target when
        random_background is.  (loss, d_raw [K, 4], mean distortion or None); the last query(train=True) is the packed one."""
        from .occupancy import WARMUP
        self._grid_for_step(update=True)
        B = rays.shape[0]
        self._march_gen.manual_seed(parallel.counter_seed(self.seed, self.rank, 4, self.it))
        jitter = torch.rand(B, dtype=torch.float32, device=self.device, generator=self._march_gen)
        offsets, rows, z, K = self.grid.march(rays, jitter, use_bits=self.it >= WARMUP)
        self.last_march = (B, K)
        raw = self._field.query_packed(rows, z, train=True)
        if self.random_background:
            if background is None:
                self._bg_gen.manual_seed(parallel.counter_seed(self.seed, self.rank, 5, self.it))
                background = torch.rand(B, 3, dtype=torch.float32, device=self.device, generator=self._bg_gen)
        dist_on = self.distortion_weight is not None
        loss, dist, d_raw, _ = render.composite_packed_train(raw, z, offsets, rays, self.grid.step_world, target, self.white_bkgd,
                                                             background, self.march_steps if dist_on else None,
                                                             self.distortion_weight if dist_on else 0.0)
        return loss, d_raw, dist

    def render_rays(self, rays: torch.Tensor, u=None, aux: bool = False, background=None):
        """rgb [B, 3] of rays [B, 11], `chunk` rays per call.  aux=True: {"rgb", "acc" [B], "depth" [B]} and, in march mode,
        "samples" [B] int32 (the samples composited per ray); with distortion_weight set (and no early termination) also
        "distortion" [B], every ray's distortion loss L_b.
        background (march mode only; None: white_bkgd decides): 3 numbers, one colour behind all rays, or a tensor [B, 3], one per
        ray.  (0, 0, 0) with aux=True gives premultiplied colour plus "acc": an RGBA frame."""
        if background is not None:
            if self.march_steps is None:
                raise ValueError("NGPTrainer.render_rays: background needs march_steps (the 64-sample renderers composite onto "
                                 "white or nothing: white_bkgd)")
            background, bg_stride = render.background_arg(background, rays.shape[0], rays.device)
        outs = []
        self._join_comm()
        if self.march_steps is not None:                     # march mode: jitter 0.5, the bitfield once the warm-up is over
            from .occupancy import WARMUP
            use_bits = self.it >= WARMUP
            for s in range(0, rays.shape[0], self.chunk):
                r = N.f32(rays[s:s + self.chunk])
                bg = background if background is None or bg_stride == 0 else background[s:s + self.chunk]
                if self.min_transmittance is not None:
                    o = self.grid.render_ert(self._field, r, 0.5, self.min_transmittance, self.white_bkgd, use_bits=use_bits,
                                             background=bg)
                    outs.append(o if aux else o["rgb"])
                    continue
                offsets, rows, z, K = self.grid.march(r, 0.5, use_bits=use_bits)
                raw = self._field.query_packed(rows, z)
                with_dist = aux and self.distortion_weight is not None
                rgb, acc, depth, dist = render.composite_packed_render(raw, z, offsets, r, self.grid.step_world, self.white_bkgd, bg,
                                                                       self.march_steps if with_dist else None)
                o = {"rgb": rgb, "acc": acc, "depth": depth, "samples": (offsets[1:] - offsets[:-1]).to(torch.int32)} if aux else rgb
                if with_dist:
                    o["distortion"] = dist
                outs.append(o)
            return _cat(outs, aux)
        for s in range(0, rays.shape[0], self.chunk):
            r = rays[s:s + self.chunk]
            z = sampling.sample_coarse(r, self.n)
            raw = self._field.query(r, z, grid=self._grid_for_step())
            rgb, _, acc, _, depth = render.composite(raw, z, r, 0.0, self.white_bkgd, need_weights=False)
            outs.append({"rgb": rgb, "acc": acc, "depth": depth} if aux else rgb)
        return _cat(outs, aux)

    def ray_distortion(self, rays: torch.Tensor) -> torch.Tensor:
        """dist [B]: the distortion loss L_b of rays [B, 11] on the one-shot march renderer's samples
        (jitter 0.5).  March mode only; works whether or not the trainer was built with a distortion_weight, so that a field
        trained without the regulariser can be measured by the same yardstick."""
        if self.march_steps is None:
            raise ValueError("NGPTrainer.ray_distortion needs march_steps (the distortion loss is defined on the march's samples)")
        from .occupancy import WARMUP
        self._join_comm()
        outs = []
        for s in range(0, rays.shape[0], self.chunk):
            r = N.f32(rays[s:s + self.chunk])
            offsets, rows, z, K = self.grid.march(r, 0.5, use_bits=self.it >= WARMUP)
            raw = self._field.query_packed(rows, z)
            outs.append(render.composite_packed_render(raw, z, offsets, r, self.grid.step_world, self.white_bkgd,
                                                       dist_steps=self.march_steps)[3])
        return torch.cat(outs, 0) if outs else torch.empty(0, dtype=torch.float32, device=self.device)

    def _grid_for_step(self, update: bool = False):
        """The occupancy grid to cull with at this iteration (None: every sample runs); update=True (the training step) first
        updates it when the iteration is a multiple of UPDATE_EVERY."""
        if self.grid is None:
            return None
        from .occupancy import UPDATE_EVERY, WARMUP
        if update and self.it % UPDATE_EVERY == 0:
            self.grid.update(self._field, self.it)
        return self.grid if self.it >= WARMUP else None

    def sync_optimizer_state(self):
        """COLLECTIVE (every rank, same iteration): with sharded table updates (table_sync "shard", world_size > 1) a rank's
        Adam moments are current on its own shards only; this gathers the others'.  A no-op otherwise.  Call it on all ranks
        before a rank-0 `state_dict()` / `save()` (entrypoints/test_nerf.py does)."""
        if self.world > 1 and self.table_sync == "shard" and "tables" in self._opt.state and not self._moments_synced:
            self._join_comm()
            per_level = self._field.enc.hash_table_size * self._field.enc.n_features_per_level
            for t in self._opt.state["tables"]:
                for lo, hi in self._field.level_groups:
                    n = (hi - lo) * per_level // self.world
                    a = lo * per_level + self.rank * n
                    torch.distributed.all_gather_into_tensor(t[lo * per_level:hi * per_level], t[a:a + n].clone())
        self._moments_synced = True

    def state_dict(self):
        """Never communicates.  With sharded table updates the Adam moments of the other ranks' shards are stale after a
        training step: raises until `sync_optimizer_state()` has run (on every rank) at this iteration."""
        if self.world > 1 and self.table_sync == "shard" and not self._moments_synced:
            raise RuntimeError("NGPTrainer.state_dict / save: the Adam moments of the hash tables are sharded across ranks "
                               "(table_sync='shard'); call tr.sync_optimizer_state() on EVERY rank first (a collective), then "
                               "save from rank 0")
        sd = super().state_dict()
        if self.grid is not None:                       # the density grid travels; the bitfield is rebuilt from it on load
            sd["extra"] = {f"occupancy/{k}": v for k, v in self.grid.state_dict().items()}
        return sd

    def load_state_dict(self, sd, allow_legacy_rng: bool = False):
        """Joins the comm stream first (the table all-gathers of a sharded step may still be writing the buffers this loads into),
        and a loaded state is complete on every rank: the moments count as synced until the next sharded step."""
        self._join_comm()
        super().load_state_dict(sd, allow_legacy_rng=allow_legacy_rng)
        self._moments_synced = True
        self._apply_level_weights()                     # not checkpointed: the weights follow from the restored `it`
        if self.grid is not None:
            self.grid.seed = int(self.seed)             # the update stream follows the adopted run's seed, like the ray streams
            occ = {k[len("occupancy/"):]: v for k, v in sd.get("extra", {}).items() if k.startswith("occupancy/")}
            if occ:
                self.grid.load_state_dict(occ)
            else:                                       # a checkpoint written without a grid: start from the all-occupied grid
                self.grid.reset()

    def _checkpoint_buffers(self):
        """Trainer.save / load / state_dict / load_state_dict work on these: the 2 x 64 MLP and the hash tables, with
        their two Adam (m, v) pairs and step counts (bias correction is on here, so the counts matter)."""
        return {"mlp": self._field.mlp, "tables": self._field.table}
