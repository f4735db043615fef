"""Occupancy grid for empty-space skipping of the hash-grid model (Instant-NGP, Mueller et al. 2022, section 4; one cascade).

The reference has no such grid; this is the standard companion of a hash-grid NeRF, opt-in through
`NGPTrainer(occupancy_grid=True)`.  Semantics (include/nerf_hip.h "occupancy grid"):

  * RES^3 float32 densities over the unit cube the hash grid sees (the field's scene box), plus a bitfield.
  * update (every UPDATE_EVERY training iterations): one jittered point per cell from a counter-based stream keyed by
    (seed, update index) -- never the rank, so all ranks build identical grids from identical tables --, sigma = raw[..., 3]
    of the current field there, density = max(density * DECAY, relu(sigma)), thr = min(THRESHOLD / delta, mean(density))
    with delta = (far - near) / n_depth_samples and the mean a fixed-order reduction, bit = density > thr.
  * The grid starts all occupied.  A sample whose cell is empty is not evaluated: its raw output is (0, 0, 0, 0).
  * The constants are module constants, not options.

Device work: nerf_occ_points -> nerf_ngp_query_fused_h (n = 1) -> nerf_occ_merge per chunk of cells, then nerf_occ_finalize;
a cull is nerf_occ_cull (+ one read of K to the host), the query of the K kept rows, nerf_scatter_rows.

March mode (`OccupancyGrid(..., march_steps=S)`, `NGPTrainer(occupancy_grid=True, march_steps=S)`; include/nerf_hip.h "ray
march"): the grid also samples.  `march()` walks each ray through the box at the fixed step
step_world = sqrt(3) / S * 2 bound and keeps the steps in occupied cells (nerf_occ_march_count, one read of K, nerf_occ_march_write).
The density of that field is trunc_exp(raw sigma), so the merge uses exp (nerf_occ_merge_ex) and the threshold cap is
THRESHOLD / step_world.

Early ray termination (`render_ert`, `NGPTrainer(..., min_transmittance=eps)`; include/nerf_hip.h "early ray termination",
DESIGN.md section 13): rendering only.  Rays are marched in rounds of a few more samples each, queried, folded serially into a
per-ray state, and dropped once their transmittance is below eps or their walk has ended.  One read of (K, live rays) per round.
"""
import math
import numbers
import time
from typing import Dict, Optional, Tuple

import torch

from .. import _native as N

LOG2_RES = 7                 # 128^3 cells
RES = 1 << LOG2_RES
DECAY = 0.95
THRESHOLD = 0.01             # thr cap = THRESHOLD / delta
UPDATE_EVERY = 16            # training iterations between updates (warm-up included)
WARMUP = 256                 # training iterations before anything is culled
_CHUNK = 1 << 19             # cells evaluated per query of an update (23 MB of rows)


MAX_MARCH_STEPS = 1024       # NERF_MARCH_MAX_STEPS
RELU, EXP = 0, 1             # NERF_OCC_RELU / NERF_OCC_EXP: the density activation of the merge


def check_march_steps(march_steps) -> int:
    """march_steps as an int in [1, MAX_MARCH_STEPS], or ValueError."""
    if isinstance(march_steps, bool) or not isinstance(march_steps, int) or not 1 <= march_steps <= MAX_MARCH_STEPS:
        raise ValueError(f"march_steps must be an int in [1, {MAX_MARCH_STEPS}], got {march_steps!r}")
    return march_steps


def check_min_transmittance(min_transmittance) -> Optional[float]:
    """None, or min_transmittance as a float in [0, 1); ValueError otherwise (NaN included)."""
    if min_transmittance is None:
        return None
    if isinstance(min_transmittance, bool) or not isinstance(min_transmittance, numbers.Real) \
            or not 0.0 <= float(min_transmittance) < 1.0:
        raise ValueError(f"min_transmittance must be None or a number in [0, 1), got {min_transmittance!r}")
    return float(min_transmittance)


def check_distortion_weight(distortion_weight) -> Optional[float]:
    """None, or distortion_weight as a finite float > 0; ValueError otherwise (0, NaN and inf included)."""
    if distortion_weight is None:
        return None
    if isinstance(distortion_weight, bool) or not isinstance(distortion_weight, numbers.Real) \
            or not 0.0 < float(distortion_weight) < math.inf:
        raise ValueError(f"distortion_weight must be None or a finite number > 0, got {distortion_weight!r}")
    return float(distortion_weight)


def march_step_world(march_steps: int, bound: float) -> float:
    """The march's world step sqrt(3) / march_steps * 2 bound, computed in double and rounded once to float32."""
    return float(torch.tensor(math.sqrt(3.0) / int(march_steps) * 2.0 * float(bound), dtype=torch.float32))


class OccupancyGrid:
    """Density grid + bitfield over `field`'s scene box (a HashNeRF built with a `bound`)."""

    def __init__(self, field, near: float, far: float, n_depth_samples: int, seed: int = 0, device=None,
                 march_steps: Optional[int] = None):
        """march_steps (None: the culling grid of section 11, unchanged): the grid of the ray march -- sample spacing
        delta = march_step_world(march_steps, bound) instead of (far - near) / n_depth_samples, and the exp density activation."""
        if getattr(field, "bound", None) is None:
            raise ValueError("OccupancyGrid: the field has no scene box (HashNeRF(bound=None) works in world coordinates); "
                             "an occupancy grid needs a bound")
        self.march_steps = None if march_steps is None else check_march_steps(march_steps)
        self.device = torch.device(device) if device is not None else field.enc.tables.device
        self.pos_scale, self.pos_offset = float(field.pos_scale), float(field.pos_offset)
        self.seed = int(seed)
        if self.march_steps is None:
            self.delta = (float(far) - float(near)) / int(n_depth_samples)
            self.activation = RELU
        else:
            self.delta = march_step_world(self.march_steps, field.bound)
            self.activation = EXP
        self.step_world = self.delta
        self.thr_cap = THRESHOLD / self.delta
        ncells = RES ** 3
        self.density = torch.zeros(ncells, dtype=torch.float32, device=self.device)
        self.bits = torch.empty(ncells // 32, dtype=torch.int32, device=self.device)
        self.thr = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.updates = 0
        self._fin_ws = torch.empty(N.lib().nerf_occ_finalize_workspace_bytes(LOG2_RES), dtype=torch.uint8, device=self.device)
        self._pts = None                    # (rays [CHUNK, 11], z [CHUNK, 1]) of the update
        self._cull = {}                     # capacity buffers of the cull, grown on demand
        self.timing = None                  # tools/ngp_occupancy.py: list receiving (name, start event, end event)
        self.last_ert = None                # render_ert: {"rounds", "marched"} of the last call
        self.reset()

    # ------------------------------------------------------------------ state
    def reset(self):
        """Density 0, every cell occupied, no update yet."""
        self.density.zero_()
        self.bits.fill_(-1)
        self.thr.zero_()
        self.updates = 0

    def occupied_fraction(self) -> float:
        """Fraction of cells whose bit is set (one host read)."""
        b = self.bits.view(torch.uint8)
        ones = sum(int(((b >> k) & 1).sum()) for k in range(8))
        return ones / float(RES ** 3)

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return {"density": self.density.detach().cpu().clone(), "updates": torch.tensor(self.updates, dtype=torch.int64)}

    def load_state_dict(self, sd):
        """The bitfield is not stored: it is rebuilt from the density (the same finalize pass, so the same bits)."""
        d = torch.as_tensor(sd["density"]).reshape(-1)
        if d.numel() != RES ** 3:
            raise ValueError(f"OccupancyGrid.load_state_dict: {d.numel()} densities, the grid has {RES ** 3}")
        self.density.copy_(d.to(self.device, torch.float32))
        self.updates = int(sd["updates"])
        if self.updates == 0:
            self.bits.fill_(-1)
            self.thr.zero_()
        else:
            self._finalize()

    # ------------------------------------------------------------------ update
    def points(self, update: int, cell0: int = 0, count: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """The jittered points of cells [cell0, cell0 + count) for update index `update`: rays [count, 11] (o = point, the rest 0)
        and z [count, 1] (0)."""
        if count is None:
            count = RES ** 3 - cell0
        rays = torch.empty(count, 11, dtype=torch.float32, device=self.device)
        z = torch.empty(count, 1, dtype=torch.float32, device=self.device)
        self._points_into(update, cell0, count, rays, z)
        return rays, z

    def _points_into(self, update, cell0, count, rays, z):
        N.check(N.lib().nerf_occ_points(LOG2_RES, cell0, count, self.seed, int(update), self.pos_scale, self.pos_offset,
                                        N.ptr(rays), N.ptr(z), N.stream()))

    def merge(self, sigma_raw: torch.Tensor, cell0: int = 0):
        """density[cell0 : cell0 + count] = max(density * DECAY, act(raw[:, 3])) for raw [count, 4] (or [count, 1, 4]); act is relu,
        or exp in march mode (a NaN counts as 0 either way)."""
        raw = N.f32(sigma_raw).reshape(-1, 4)
        count = raw.shape[0]
        assert 0 <= cell0 and cell0 + count <= self.density.numel()
        dens = N.ptr(self.density[cell0:cell0 + count]) if count else None
        if self.activation == RELU:
            N.check(N.lib().nerf_occ_merge(dens, N.ptr(raw) if count else None, count, DECAY, N.stream()))
        else:
            N.check(N.lib().nerf_occ_merge_ex(dens, N.ptr(raw) if count else None, count, DECAY, self.activation, N.stream()))

    def _finalize(self):
        N.check(N.lib().nerf_occ_finalize(N.ptr(self.density), LOG2_RES, self.thr_cap, N.ptr(self._fin_ws), N.ptr(self.thr),
                                          N.ptr(self.bits), N.stream()))

    def update(self, field, it: int):
        """One update from the current `field` (a HashNeRF), keyed by (seed, it // UPDATE_EVERY)."""
        ncells = RES ** 3
        if self._pts is None:
            self._pts = (torch.empty(_CHUNK, 11, dtype=torch.float32, device=self.device),
                         torch.empty(_CHUNK, 1, dtype=torch.float32, device=self.device))
        u = int(it) // UPDATE_EVERY
        for c0 in range(0, ncells, _CHUNK):
            cnt = min(_CHUNK, ncells - c0)
            rays, z = self._pts[0][:cnt], self._pts[1][:cnt]
            self._points_into(u, c0, cnt, rays, z)
            raw = field.query(rays, z)                     # inference query: the training activations are not touched
            self.merge(raw, c0)
        self._finalize()
        self.updates += 1

    # ------------------------------------------------------------------ cull
    def _buf(self, key, shape, dtype):
        t = self._cull.get(key)
        n = 1
        for s in shape:
            n *= s
        if t is None or t.numel() < n:
            t = torch.empty(n, dtype=dtype, device=self.device)
            self._cull[key] = t
        return t[:n].view(*shape)

    def cull(self, rays: torch.Tensor, z: torch.Tensor, raw: Optional[torch.Tensor] = None):
        """(idx [K] int64, rays_k [K, 11], z_k [K, 1], raw [B, n, 4]) for rays [B, 11], z [B, n]: the kept samples in ray-major
        order, their ray rows and depths, and raw with (0, 0, 0, 0) at every culled sample (the kept rows unwritten).  One read
        of K to the host.  rays_k / z_k / idx are views of buffers the next cull overwrites."""
        rays, z = N.f32(rays), N.f32(z)
        B, n = z.shape
        M = B * n
        if raw is None:
            raw = torch.empty(B, n, 4, dtype=torch.float32, device=self.device)
        if self.timing is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        ws = self._buf("ws", (max(1, N.lib().nerf_occ_cull_workspace_bytes(B, n)),), torch.uint8)
        idx = self._buf("idx", (M,), torch.int64)
        cnt = self._buf("count", (1,), torch.int64)
        rk = self._buf("rays", (M, 11), torch.float32)
        zk = self._buf("z", (M, 1), torch.float32)
        N.check(N.lib().nerf_occ_cull(N.ptr(rays), N.ptr(z), B, n, N.ptr(self.bits), LOG2_RES, self.pos_scale, self.pos_offset,
                                      N.ptr(ws), N.ptr(idx), N.ptr(cnt), N.ptr(rk), N.ptr(zk), N.ptr(raw), N.stream()))
        if self.timing is not None:
            e1.record()
            self.timing.append(("cull", e0, e1))
        if self.timing is not None:
            t0 = time.perf_counter()
        K = int(cnt.item())                                # the one host sync of a culled query
        if self.timing is not None:
            self.timing.append(("sync_host", (time.perf_counter() - t0) * 1e3))
        return idx[:K], rk[:K], zk[:K], raw, K


    # ------------------------------------------------------------------ march
    def _grow(self, key, n, dtype):
        """A capacity buffer of at least n elements (grown by 1.25 x, so that a slowly rising K does not reallocate every step)."""
        t = self._cull.get(key)
        if t is None or t.numel() < n:
            t = torch.empty(max(n, int(1.25 * (t.numel() if t is not None else 0))), dtype=dtype, device=self.device)
            self._cull[key] = t
        return t[:n]

    def march(self, rays: torch.Tensor, jitter, use_bits: bool = True):
        """(offsets [B + 1] int64, rows [K, 11], z [K], K) of the march of rays [B, 11] (march mode only): ray b owns the packed
        samples [offsets[b], offsets[b + 1]).  jitter: float32 [B] per ray, or one float for every ray (0.5 when rendering).
        use_bits=False (the warm-up) keeps every step inside the box.  One read of K to the host; the outputs are views of
        buffers the next march overwrites."""
        if self.march_steps is None:
            raise ValueError("OccupancyGrid.march: the grid was built without march_steps")
        rays = N.f32(rays)
        B = rays.shape[0]
        if torch.is_tensor(jitter):
            jit, jc = N.f32(jitter).reshape(-1), 0.0
            assert jit.numel() == B, "march: one jitter per ray"
        else:
            jit, jc = None, float(jitter)
        if self.timing is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        ws = self._grow("march_ws", max(1, N.lib().nerf_occ_march_workspace_bytes(B)), torch.uint8)
        offsets = self._grow("march_offsets", B + 1, torch.int64)
        args = (N.ptr(rays) if B else None, B, N.ptr(jit) if B else None, jc, N.ptr(self.bits) if use_bits else None, LOG2_RES,
                self.pos_scale, self.pos_offset, self.step_world, self.march_steps, N.ptr(ws), N.ptr(offsets))
        N.check(N.lib().nerf_occ_march_count(*args, N.stream()))
        if self.timing is not None:
            t0 = time.perf_counter()
        K = int(offsets[B].item())                          # the one host sync of a march
        if self.timing is not None:
            self.timing.append(("sync_host", (time.perf_counter() - t0) * 1e3))
        rows = self._grow("march_rows", max(1, K) * 11, torch.float32)[:K * 11].view(K, 11)
        z = self._grow("march_z", max(1, K), torch.float32)[:K]
        N.check(N.lib().nerf_occ_march_write(*args, N.ptr(rows) if K else N.ptr(self._cull["march_rows"]),
                                             N.ptr(z) if K else N.ptr(self._cull["march_z"]), N.stream()))
        if self.timing is not None:
            e1.record()
            self.timing.append(("march", e0, e1))
        return offsets, rows, z, K


    # ------------------------------------------------------------------ early ray termination
    def _ert_state(self, B: int):
        """(istate [B, 4] int32, fstate [B, 6] float32, live [B] int32, live [B] int32): the round renderer's state buffers."""
        n = max(1, B)
        return (self._grow("ert_istate", 4 * n, torch.int32)[:4 * B].view(B, 4),
                self._grow("ert_fstate", 6 * n, torch.float32)[:6 * B].view(B, 6),
                self._grow("ert_live0", n, torch.int32)[:B], self._grow("ert_live1", n, torch.int32)[:B])

    def _jitter(self, jitter, B):
        if torch.is_tensor(jitter):
            jit = N.f32(jitter).reshape(-1)
            assert jit.numel() == B, "march: one jitter per ray"
            return jit, 0.0
        return None, float(jitter)

    def march_resume(self, rays, jitter, istate, live, A: int, max_new: int, live_out, use_bits: bool = True):
        """One round of the resumed march (`nerf_ert_march_count`, one read of (K, A') to the host, `nerf_ert_march_write`): each
        of the A rays live[:A] takes up to max_new further kept samples from its saved (k, kept) = istate[b, 0:2], which is
        advanced.  (offsets [A + 1], rows [K, 11], z [K], K, A'), the A' rays still live in live_out[:A'].  The outputs are views
        of buffers the next round overwrites."""
        rays = N.f32(rays)
        B = rays.shape[0]
        jit, jc = self._jitter(jitter, B)
        ws = self._grow("ert_ws", max(1, N.lib().nerf_ert_march_workspace_bytes(B)), torch.uint8)
        tot = self._grow("ert_totals", 2, torch.int64)
        offsets = self._grow("ert_offsets", A + 1, torch.int64)
        head = (N.ptr(rays) if B else None, B, N.ptr(jit) if jit is not None and B else None, jc,
                N.ptr(self.bits) if use_bits else None, LOG2_RES, self.pos_scale, self.pos_offset, self.step_world, self.march_steps,
                N.ptr(live) if A else None, A)
        N.check(N.lib().nerf_ert_march_count(*head, N.ptr(istate) if A else None, int(max_new), N.ptr(ws), N.ptr(tot), N.stream()))
        if self.timing is not None:
            t0 = time.perf_counter()
        K, A_next = tot.tolist()                             # the one host read of a round
        if self.timing is not None:
            self.timing.append(("sync_host", (time.perf_counter() - t0) * 1e3))
        rows = self._grow("ert_rows", max(1, K) * 11, torch.float32)
        zb = self._grow("ert_z", max(1, K), torch.float32)
        if K:
            N.check(N.lib().nerf_ert_march_write(*head, N.ptr(istate), int(max_new), N.ptr(ws), N.ptr(offsets), N.ptr(live_out),
                                                 N.ptr(rows), N.ptr(zb), N.stream()))
        return offsets, rows[:K * 11].view(K, 11), zb[:K], K, A_next

    def render_ert(self, field, rays, jitter, min_transmittance: float, white_bkgd: bool = False, use_bits: bool = True,
                   slots: int = 8, background=None) -> Dict[str, torch.Tensor]:
        """Render rays [B, 11] through `field` (a HashNeRF) with early ray termination at T < min_transmittance (march mode only).
        Round r gives each live ray m_r = min(march_steps, max(1, slots B // A)) slots, A the rays live before it (slots is a
        tuning knob: by the fold's order no output depends on it).  {"rgb" [B, 3], "acc" [B], "depth" [B], "samples" [B] int32};
        self.last_ert = {"rounds", "marched"} of the call (marched: samples queried, terminated rays' surplus included).
        background (None: white_bkgd decides): 3 numbers or a tensor [B, 3], the colour behind the rays (`nerf_ert_finish_bg`)."""
        if self.march_steps is None:
            raise ValueError("OccupancyGrid.render_ert: the grid was built without march_steps")
        eps = check_min_transmittance(min_transmittance)
        if eps is None:
            raise ValueError("OccupancyGrid.render_ert: min_transmittance is required")
        if int(slots) < 1:
            raise ValueError(f"OccupancyGrid.render_ert: slots must be >= 1, got {slots!r}")
        from ..rendering import render
        rays = N.f32(rays)
        B = rays.shape[0]
        istate, fstate, la, lb = self._ert_state(B)
        render.ert_init(istate, fstate, la, B)
        A, rounds, total = B, 0, 0
        while A > 0:
            m = min(self.march_steps, max(1, int(slots) * B // A))
            offsets, rows, z, K, A_next = self.march_resume(rays, jitter, istate, la, A, m, lb, use_bits=use_bits)
            if K == 0:
                break
            raw = field.query_packed(rows, z)
            render.ert_fold(raw, z, offsets, la, A, istate, fstate, self.step_world, eps)
            A, la, lb = A_next, lb, la
            rounds += 1
            total += K
        rgb, acc, depth, samples = render.ert_finish_over(istate, fstate, white_bkgd, background)
        self.last_ert = {"rounds": rounds, "marched": total}
        return {"rgb": rgb, "acc": acc, "depth": depth, "samples": samples}


def scatter_rows(src: torch.Tensor, idx: torch.Tensor, dst: torch.Tensor):
    """dst.view(-1, C)[idx] = src.view(-1, C) in place (`nerf_scatter_rows`)."""
    C_ = src.shape[-1]
    src = N.f32(src).reshape(-1, C_)
    d2 = dst.view(-1, C_)
    N.check(N.lib().nerf_scatter_rows(N.ptr(src) if src.shape[0] else None, N.ptr(idx) if idx.numel() else None, idx.numel(),
                                      C_, N.ptr(d2), d2.shape[0], N.stream()))
    return dst


def gather_rows(src: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """src.view(-1, C)[idx] (`nerf_gather_rows`)."""
    C_ = src.shape[-1]
    s2 = N.f32(src).reshape(-1, C_)
    out = torch.empty(idx.numel(), C_, dtype=torch.float32, device=src.device)
    if idx.numel():
        N.check(N.lib().nerf_gather_rows(N.ptr(s2), s2.shape[0], N.ptr(idx), idx.numel(), C_, N.ptr(out), N.stream()))
    return out
