"""End-to-end oracle of one march-mode training step (a helper module for the tests, not a conftest; NGPTrainer._march_step_forward
and NGPTrainer.train_step in engine/ngp.py are the product).  It composes what the repository already has and adds no arithmetic
of its own:

  positions   x = (o + z d) pos_scale + pos_offset of the packed samples (rows [K, 11], z [K])
  features    oracle.hashgrid_encoding per level, times the level weights | oracle.sh_encoding(viewdirs, 3)
  network     oracle.nerf_forward on OracleNGP's NerfArch (2 x 64, 32 + 16 inputs, view head)
  compositing tests/_march_ref.composite (TruncExp density), or tests/_background_ref.composite / target over a per-ray background
  objective   MSE + weight * mean_b L_b with tests/_distortion_ref.losses

in float64 (or, to size the bars, the same graph in float32), the tables and the flat MLP parameters as autograd leaves.  The
gradient is taken in the two stages the trainer has -- d_raw = d objective / d raw, then (g_mlp, g_tab) = raw's vector-Jacobian
product with d_raw -- which is the chain rule, not another formula; with emulate_bf16 the second stage rounds like the kernels.

MUTATIONS are wrong wirings of the chain that would still train and still be bit-reproducible.  `step(..., mutate=name)` computes
what a trainer with that mistake would; tests/test_march_step_ref_host.py shows that the bars of tests/test_gpu_march_step.py
tell every one of them from rounding.  This module imports nothing from the package under test.
"""
import torch

from oracle import nerf_oracle as O
from tests import _background_ref as BG
from tests import _distortion_ref as D
from tests import _march_ref as M

ARCH = O.NerfArch(channel_input=32, channel_input_views=16, n_layers=2, width=64, skips=(), use_viewdirs=True)
MASK_LAYERS = (("pos0", 0), ("pos1", 1), ("dir0", 9))        # nerf_forward's name, debug_layer's index

MUTATIONS = (
    "dist_sum",              # the distortion term summed over rays instead of averaged
    "dist_dropped",          # the distortion term dropped
    "dist_steps_x2",         # march_steps of the distortion positions off by a factor 2
    "step_world_x2",         # step_world from march_steps * 2
    "bg_render_only",        # the background added to the rendered colour but not to the target
    "bg_target_only",        # ... and the reverse
    "alpha_premultiplied",   # straight alpha treated as premultiplied in the target
    "lw_forward_only",       # level weights applied in the forward only (not to the gradient)
    "lw_twice",              # level weights applied twice to the gradient
    "lw_rounded",            # fractional level weights rounded to 0 / 1
    "d_raw_shifted",         # d_raw shifted by one row after every ray without samples
    "no_pos_offset",         # pos_offset omitted
    "prev_table_grad",       # the previous batch's table gradient added
)


def init_tables(n_levels: int, log2_T: int, F: int, scale: float, seed: int) -> torch.Tensor:
    """The tables MultiHashEncoding starts from: U(-scale, scale) from the seeded CPU stream, float32 [L, T, F]."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(n_levels, 1 << log2_T, F, generator=g) * 2 - 1) * scale


def init_mlp(seed: int) -> torch.Tensor:
    """The flat 2 x 64 parameters OracleNGP and the device model start from (float32 [13188])."""
    return O.flatten_params(ARCH, O.init_params(ARCH, seed))


def unit_positions(rows, z, pos_scale, pos_offset, dtype=torch.float64):
    rows, z = rows.to(dtype), z.to(dtype)
    return (rows[:, 0:3] + z[:, None] * rows[:, 3:6]) * pos_scale + pos_offset


def touched(x: torch.Tensor, res, T: int) -> torch.Tensor:
    """bool [L, T]: the table entries some corner of some sample x [K, 3] hashes to (the corners of oracle.hashgrid_encoding)."""
    out = torch.zeros(len(res), T, dtype=torch.bool)
    for l, r in enumerate(res):
        xs = x.double() * float(r)
        fl, ce = torch.floor(xs).to(torch.int64), torch.ceil(xs).to(torch.int64)
        for cx in (0, 1):
            for cy in (0, 1):
                for cz in (0, 1):
                    g = torch.stack([ce[:, 0] if cx else fl[:, 0], ce[:, 1] if cy else fl[:, 1], ce[:, 2] if cz else fl[:, 2]], -1)
                    out[l, O.hash_coords(g, T)] = True
    return out


class _Scaled(torch.autograd.Function):
    """x * fwd in the forward, gradient * bwd in the backward: the level weights as a mis-wired scatter would see them (the
    right wiring has bwd == fwd and is not routed through here)."""

    @staticmethod
    def forward(ctx, x, fwd, bwd):
        ctx.save_for_backward(bwd)
        return x * fwd

    @staticmethod
    def backward(ctx, g):
        (bwd,) = ctx.saved_tensors
        return g * bwd, None, None


def _shift_rows(d_raw: torch.Tensor, offsets) -> torch.Tensor:
    """d_raw with its rows moved down by one after every ray without samples (zeros shifted in, the tail dropped)."""
    offs = [int(v) for v in offsets]
    out = torch.zeros_like(d_raw)
    shift = 0
    for b in range(len(offs) - 1):
        lo, hi = offs[b], offs[b + 1]
        if hi == lo:
            shift += 1
            continue
        dst_lo, dst_hi = min(lo + shift, d_raw.shape[0]), min(hi + shift, d_raw.shape[0])
        out[dst_lo:dst_hi] = d_raw[lo:lo + (dst_hi - dst_lo)]
    return out


def _objective(raw, offsets, z, rays, target, background, step_world, march_steps, dist_weight, mutate=None):
    """(MSE, mean_b L_b, objective, rgb [B, 3]) of raw [K, 4] in raw's dtype: the compositing references and the loss, wired as
    the trainer wires them (or, with `mutate`, mis-wired)."""
    dtype = raw.dtype
    zz = z.to(dtype)
    if torch.is_tensor(background):
        bg = background.detach().cpu().to(dtype)
        if mutate == "bg_target_only":
            rgb = M.composite(raw, zz, offsets, step_world, False)[0]
        else:
            rgb = BG.composite(raw, zz, offsets, step_world, bg)[0]
        if mutate == "bg_render_only":
            want = target[:, :3] * target[:, 3:4]
        elif mutate == "alpha_premultiplied":
            want = target[:, :3] + bg * (1.0 - target[:, 3:4])
        else:
            want = BG.target(target, bg)
    else:
        assert background in (None, "white") and target.shape[1] == 3
        rgb = M.composite(raw, zz, offsets, step_world, background == "white")[0]
        want = target
    mse = ((rgb - want) ** 2).mean()
    objective, dist = mse, raw.new_zeros(())
    if dist_weight:
        per_ray = D.losses(raw, z, offsets, rays, step_world, march_steps * (2 if mutate == "dist_steps_x2" else 1))
        dist = per_ray.mean()
        if mutate == "dist_sum":
            objective = mse + dist_weight * per_ray.sum()
        elif mutate != "dist_dropped":
            objective = mse + dist_weight * dist
    return mse, dist, objective, rgb


def given_raw(raw, offsets, z, rays, target, background, step_world: float, march_steps: int, dist_weight, dtype=torch.float64):
    """{"loss", "dist", "d_raw"} of the compositing and loss links alone, evaluated at somebody's raw [K, 4] (the kernel's own):
    whatever the network's precision, these links are float32 kernels and are held to float32 bars in every arm."""
    cpu = lambda t: t.detach().cpu()
    r = cpu(raw).reshape(-1, 4).to(dtype).requires_grad_(True)
    mse, dist, objective, _ = _objective(r, cpu(offsets), cpu(z), cpu(rays), cpu(target).to(dtype), background, step_world,
                                         march_steps, dist_weight)
    d_raw = torch.autograd.grad(objective, r)[0] if r.shape[0] else r.new_zeros(0, 4)
    return {"loss": mse.detach(), "dist": dist.detach(), "d_raw": d_raw}


def step(offsets, rows, z, rays, target, background, step_world: float, march_steps: int, dist_weight, level_weights,
         tables, res, p_flat, pos_scale: float, pos_offset: float, masks=None, emulate_bf16: bool = False,
         dtype=torch.float64, mutate=None, prev_g_tab=None, taps=None):
    """One step's forward and gradients.  offsets [B + 1], rows [K, 11], z [K]: the packed samples; rays [B, 11]; target [B, 3],
    or straight RGBA [B, 4] with a background [B, 3]; background None (nothing behind the rays), "white" or [B, 3]; dist_weight
    None / 0 (no regulariser) or > 0; level_weights None or L numbers; tables [L, T, F]; res the L resolutions; p_flat [13188];
    masks {layer: bool [K, width]} the ReLU decisions to use (None: the oracle's own); taps: a dict that receives nerf_forward's
    post-activation outputs.  dtype float64, or float32 for the same
    graph in float32.  Returns {"loss" (the MSE), "dist" (mean_b L_b, 0 without the regulariser), "raw" [K, 4], "d_raw" [K, 4],
    "g_mlp" [13188], "g_tab" [L, T, F], "rgb" [B, 3]}, detached, in dtype."""
    assert mutate is None or mutate in MUTATIONS, mutate
    cpu = lambda t: t.detach().cpu()
    offsets, rows, z, rays, target = cpu(offsets), cpu(rows), cpu(z), cpu(rays), cpu(target).to(dtype)
    tables = cpu(tables).to(dtype).requires_grad_(True)
    p = cpu(p_flat).to(dtype).requires_grad_(True)
    L, T, F = tables.shape
    K = rows.shape[0]
    if mutate == "step_world_x2":
        step_world = M.step_world(2 * march_steps, 1.0) / M.step_world(march_steps, 1.0) * step_world
    x = unit_positions(rows, z, pos_scale, 0.0 if mutate == "no_pos_offset" else pos_offset, dtype)
    feat = O.hashgrid_encoding(x, tables, res)                                   # [K, L F]
    if level_weights is not None:
        lw = torch.as_tensor([float(w) for w in level_weights], dtype=dtype)
        if mutate == "lw_rounded":
            lw = torch.round(lw)
        lw = lw.repeat_interleave(F)[None, :]
        if mutate == "lw_forward_only":
            feat = _Scaled.apply(feat, lw, torch.ones_like(lw))
        elif mutate == "lw_twice":
            feat = _Scaled.apply(feat, lw, lw * lw)
        else:
            feat = feat * lw
    shf = O.sh_encoding(rows[:, 8:11].to(dtype), 3)
    raw = O.nerf_forward(ARCH, O.unflatten_params(ARCH, p), torch.cat([feat, shf], -1), emulate_bf16, masks=masks, taps=taps)
    mse, dist, objective, rgb = _objective(raw, offsets, z, rays, target, background, step_world, march_steps, dist_weight, mutate)
    if K:
        (d_raw,) = torch.autograd.grad(objective, raw, retain_graph=True)
        if mutate == "d_raw_shifted":
            d_raw = _shift_rows(d_raw, offsets)
        g_mlp, g_tab = torch.autograd.grad(raw, [p, tables], grad_outputs=d_raw)
    else:
        d_raw, g_mlp, g_tab = raw.new_zeros(0, 4), torch.zeros_like(p), torch.zeros_like(tables)
    if mutate == "prev_table_grad":
        g_tab = g_tab + cpu(prev_g_tab).to(dtype)
    return {"loss": mse.detach(), "dist": dist.detach(), "raw": raw.detach(), "d_raw": d_raw.detach(), "g_mlp": g_mlp.detach(),
            "g_tab": g_tab.detach(), "rgb": rgb.detach()}


def objective_value(out, dist_weight) -> float:
    """MSE + weight * mean_b L_b of a `step` result."""
    return float(out["loss"]) + (float(dist_weight) * float(out["dist"]) if dist_weight else 0.0)


def rel_l2(a, b) -> float:
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def rel_max(a, b) -> float:
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def rel_abs(a, b) -> float:
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-30)


def live_levels(level_weights, L: int):
    return [l for l in range(L) if level_weights is None or float(level_weights[l]) != 0.0]


def errors(got, want, level_weights=None):
    """{quantity: relative error} of a step result `got` against the oracle's `want`: loss and dist relative, raw relative to its
    max, d_raw, g_mlp, g_tab rel-L2, g_tab_l<l> rel-L2 of every level whose weight is not 0."""
    L = want["g_tab"].shape[0]
    e = {"loss": rel_abs(got["loss"], want["loss"]), "raw": rel_max(got["raw"].reshape(-1, 4), want["raw"]),
         "d_raw": rel_l2(got["d_raw"].reshape(-1, 4), want["d_raw"]), "g_mlp": rel_l2(got["g_mlp"], want["g_mlp"]),
         "g_tab": rel_l2(got["g_tab"], want["g_tab"])}
    if float(want["dist"]) != 0.0:
        e["dist"] = rel_abs(got["dist"], want["dist"])
    for l in live_levels(level_weights, L):
        e[f"g_tab_l{l}"] = rel_l2(got["g_tab"][l], want["g_tab"][l])
    return e


# The project's bars for the quantities it already holds an end-to-end path to (tests/test_gpu_round5.py at precision 22,
# tests/test_gpu_parity.py at precision 16); d_raw, dist and the per-level table gradients take the neighbouring figure, or
# 8 x the float32 oracle's own error against float64 where that is larger (bars()).
PROJECT = {22: {"loss": 1e-3, "raw": 1e-4, "grad": 1e-3, "track": 2e-2}, 16: {"loss": 2e-2, "raw": 1e-2, "grad": 5e-2, "track": 0.25}}
F32_FACTOR = 8.0             # a 22-bit operand carries two bits fewer than float32 (x 4), doubled for margin


def bars(precision: int, f32_err):
    """{quantity: bar} for every key of f32_err = errors(float32 oracle, float64 oracle).  loss, raw, g_mlp and g_tab carry the
    project's figures as they stand; d_raw, dist and g_tab_l<l> the larger of the neighbouring project figure and F32_FACTOR
    times the float32 oracle's error.  Nothing here looks at a kernel's output."""
    P = PROJECT[precision]
    out = {}
    for k, e in f32_err.items():
        if k == "loss":
            out[k] = P["loss"]
        elif k == "raw":
            out[k] = P["raw"]
        elif k in ("g_mlp", "g_tab"):
            out[k] = P["grad"]
        elif k == "dist":
            out[k] = max(P["loss"], F32_FACTOR * e)
        else:                                                # d_raw, g_tab_l<l>
            out[k] = max(P["grad"], F32_FACTOR * e)
    return out


# ---- the inputs of tests/test_gpu_march_step.py, rebuilt on the CPU by tests/test_march_step_ref_host.py
SHAPE = dict(H=16, W=16, n_train=4, N_rand=64, march_steps=64, near=2.0, far=6.0, bound=1.5, seed=4, log2_res=7)
HASH = dict(n_levels=16, min_res=4, max_res=128, n_features_per_level=2, log2_hashmap_size=10, hash_init_scale=0.5)
DIST_WEIGHT = 0.1
LEVEL_ANNEAL = (4, 1000)
POS_SCALE, POS_OFFSET = 1.0 / (2.0 * SHAPE["bound"]), 0.5
HALF_SPACE = (0.6, 0.8, 0.0, 0.75)                           # occupied: n . c <= t over the cell centres c in [0, 1]^3; (nx, ny, nz, t)


def half_space_cells(log2_res: int = SHAPE["log2_res"]) -> torch.Tensor:
    """bool [R^3] (x fastest, the cell order of tests/_occupancy_ref.py): the hand-made occupancy of the culled arms."""
    R = 1 << log2_res
    c = (torch.arange(R, dtype=torch.float64) + 0.5) / R
    zc, yc, xc = torch.meshgrid(c, c, c, indexing="ij")
    nx, ny, nz, t = HALF_SPACE
    return (nx * xc + ny * yc + nz * zc <= t).reshape(-1)


def all_rays(poses, K, H: int, W: int, near: float, far: float) -> torch.Tensor:
    """rays [N H W, 11] of every pixel of every pose, float32 (oracle.get_rays / pack_rays)."""
    out = []
    for c2w in poses:
        ro, rd = O.get_rays(H, W, K, c2w[:3, :4])
        out.append(O.pack_rays(ro.reshape(-1, 3).float(), rd.reshape(-1, 3).float(), near, far))
    return torch.cat(out, 0)


def batch(imgs, poses, K, index: int, rgba: bool):
    """(rays [B, 11], target [B, 3 or 4], background [B, 3] or None) of batch `index`: N_rand seeded pixels over all images.  Two
    rays are edited so that the conditions on the samples hold whatever the jitter: ray 0's far plane is pulled in to its entry
    into the scene box (it meets nothing), and the far plane of the first ray whose entry lies well inside the occupied half-space
    to one march step behind the entry (z_0 = t0 + j dt < far <= z_1 for every j in [0, 1): exactly one sample).  The synthetic
    scene's alpha is 0 or 1, at which straight and premultiplied colours coincide and (1 - a) bg is bg or nothing: the RGBA
    target gets a seeded alpha in [0.1, 0.9] and seeded colours where the scene has none."""
    S = SHAPE
    rays = all_rays(poses, K, S["H"], S["W"], S["near"], S["far"])
    pix = imgs.reshape(-1, imgs.shape[-1]).cpu().float()
    g = torch.Generator().manual_seed(1000 * S["seed"] + index)
    sel = torch.randperm(rays.shape[0], generator=g)[:S["N_rand"]]
    rays, target = rays[sel].clone(), pix[sel].clone()
    t0, t1, dt, ok = M.interval(rays, POS_SCALE, POS_OFFSET, M.step_world(S["march_steps"], S["bound"]))
    nx, ny, nz, t = HALF_SPACE
    n = torch.tensor([nx, ny, nz], dtype=torch.float64)
    inside = ok & (t1 - t0 > 8 * dt)
    for s in (0.0, 1.0):                                      # both ends of the first step, 0.1 inside the plane
        x = (rays[:, 0:3] + (t0 + s * dt)[:, None] * rays[:, 3:6]).double() * POS_SCALE + POS_OFFSET
        inside = inside & ((x * n).sum(1) <= t - 0.1)
    inside[0] = False
    one = int(torch.nonzero(inside)[0])
    assert bool(ok[0])
    rays[0, 7] = t0[0]                                        # far == entry: the interval is empty
    rays[one, 7] = t0[one] + dt[one]
    bg = None
    if rgba:
        bg = torch.rand(S["N_rand"], 3, generator=g)
        a = target[:, 3:4]
        colour = torch.where(a > 0, target[:, :3], torch.rand(S["N_rand"], 3, generator=g))
        target = torch.cat([colour, 0.1 + 0.8 * (0.5 * a + 0.5 * torch.rand(S["N_rand"], 1, generator=g))], 1)
    return rays, target, bg
