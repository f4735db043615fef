"""The end-to-end oracle of the march-mode step (tests/_march_step_ref.py) held to account on the CPU, before
tests/test_gpu_march_step.py holds the trainer to it:

  * its gradients are the central differences of its own float64 objective (ReLU decisions pinned, raw sigma < 15 so that
    TruncExp's backward is the true derivative);
  * with the options off it reduces to the pieces OracleNGP and tests/_march_ref.py already have;
  * every wrong wiring of _march_step_ref.MUTATIONS moves a checked quantity by at least 10 x the bar the GPU test applies to it,
    on the GPU test's own rays, targets, backgrounds, tables and parameters (packed samples from tests/_march_ref.march on the
    hand-made half-space occupancy; only the jitter is the CPU's own stream instead of the device's).
"""
import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests import _levels_ref as LV
from tests import _march_ref as M
from tests import _march_step_ref as S

STEP = M.step_world(64, 1.5)


# ---------------------------------------------------------------- the tiny case: 6 rays, counts 0 1 2 5 0 3, 4 levels of 2^6
COUNTS = (0, 1, 2, 5, 0, 3)
TINY_RES = (4, 7, 12, 20)
TINY_LW = (1.0, 1.0, 0.375, 0.0)


def _tiny(**over):
    g = torch.Generator().manual_seed(11)
    B = len(COUNTS)
    o = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=-1) * 4.0
    d = -o / 4.0 + 0.15 * torch.randn(B, 3, generator=g)
    rays = O.pack_rays(o, d, 2.0, 6.0)
    offsets = torch.tensor([0] + list(np.cumsum(COUNTS)), dtype=torch.int64)
    rows = torch.cat([rays[b:b + 1].expand(n, 11) for b, n in enumerate(COUNTS)], 0)
    z = torch.cat([3.2 + STEP * (torch.arange(n) * (1 + b % 2) + torch.rand(1, generator=g)) for b, n in enumerate(COUNTS)]).float()
    target = torch.rand(B, 4, generator=g)
    target[:, 3] = 0.1 + 0.8 * target[:, 3]
    case = dict(offsets=offsets, rows=rows, z=z, rays=rays, target=target, background=torch.rand(B, 3, generator=g),
                step_world=STEP, march_steps=64, dist_weight=0.5, level_weights=TINY_LW,
                tables=(torch.rand(4, 64, 8, generator=g) * 2 - 1) * 0.5, res=TINY_RES, p_flat=S.init_mlp(3),
                pos_scale=S.POS_SCALE, pos_offset=S.POS_OFFSET)
    case.update(over)
    return case


def _pinned(case):
    taps = {}
    S.step(**case, taps=taps)
    return {n: taps[n].detach() > 0 for n, _ in S.MASK_LAYERS}


def test_gradients_are_the_central_differences_of_the_objective():
    """h = 1e-6 of the tensor's largest entry and an error below 1e-6 of the gradient's max-norm: what float64 gives (truncation
    ~h^2, rounding ~2^-53 |f| / h = 1e-10 at |f| = 0.03: one to three orders below the bar at max|g| of 2e-2 and 1e-4)."""
    case = _tiny()
    masks = _pinned(case)
    base = S.step(**case, masks=masks)
    assert float(base["raw"][:, 3].max()) < 15.0, "TruncExp's backward is clamped here: not the derivative"
    x = S.unit_positions(case["rows"], case["z"], S.POS_SCALE, S.POS_OFFSET)
    hit = S.touched(x, TINY_RES, 64)
    assert hit.any(1).all() and not hit.all(1).any()
    rng = np.random.default_rng(5)
    live = torch.tensor([w != 0 for w in TINY_LW])

    def value(name, idx, delta):
        c = dict(case)
        t = c[name].double().clone()
        t.view(-1)[idx] += delta
        c[name] = t
        return S.objective_value(S.step(**c, masks=masks), c["dist_weight"])

    worst = {}
    for name, grad, pool in (("p_flat", base["g_mlp"], torch.nonzero(base["g_mlp"] != 0)[:, 0]),
                             ("tables", base["g_tab"], torch.nonzero((hit & live[:, None])[:, :, None].expand(4, 64, 8).reshape(-1))[:, 0])):
        probes = rng.choice(pool.numpy(), size=40, replace=False)
        scale, h = float(grad.abs().max()), 1e-6 * float(case[name].abs().max())
        assert scale > 1e-6
        err = 0.0
        for i in probes:
            fd = (value(name, int(i), h) - value(name, int(i), -h)) / (2 * h)
            err = max(err, abs(fd - float(grad.reshape(-1)[i])) / scale)
        worst[name] = err
        assert err < 1e-6, (name, err)
    cold = torch.nonzero((~hit)[:, :, None].expand(4, 64, 8).reshape(-1))[:, 0]
    for i in rng.choice(cold.numpy(), size=5, replace=False):
        assert float(base["g_tab"].reshape(-1)[i]) == 0.0
        assert value("tables", int(i), 1e-3) == value("tables", int(i), -1e-3)
    assert bool((base["g_tab"][3] == 0).all()), "a level with weight 0 has no gradient"
    print(f"[march-step oracle] central differences: worst error / max|g| p {worst['p_flat']:.1e}, tables {worst['tables']:.1e}")


def test_options_off_reduce_to_the_packed_mse_reference():
    case = _tiny(background=None, dist_weight=None, level_weights=None)
    case["target"] = case["target"][:, :3]
    out = S.step(**case)
    loss, d_raw = M.mse_backward(out["raw"], case["offsets"], STEP, case["target"], False)
    assert abs(float(out["loss"]) - float(loss)) <= 1e-15 * float(loss)
    assert S.rel_max(out["d_raw"], d_raw) < 1e-14
    ones = S.step(**dict(case, level_weights=(1.0,) * 4))
    for k in ("loss", "raw", "d_raw", "g_mlp", "g_tab"):
        assert torch.equal(ones[k], out[k]), k


def test_a_ray_without_samples_adds_its_background_error_and_no_gradient():
    case = _tiny()
    full = S.step(**case)
    keep = [b for b, n in enumerate(COUNTS) if n > 0]
    sub = dict(case, rays=case["rays"][keep], target=case["target"][keep], background=case["background"][keep],
               offsets=torch.tensor([0] + list(np.cumsum([COUNTS[b] for b in keep])), dtype=torch.int64))
    part = S.step(**sub)
    B, Bk = len(COUNTS), len(keep)
    empty = [b for b, n in enumerate(COUNTS) if n == 0]
    t, bg = case["target"].double(), case["background"].double()
    want = sum(float(((bg[b] - (t[b, :3] * t[b, 3] + bg[b] * (1 - t[b, 3]))) ** 2).sum()) for b in empty)
    assert abs(float(full["loss"]) * 3 * B - float(part["loss"]) * 3 * Bk - want) < 1e-13
    assert abs(float(full["dist"]) * B - float(part["dist"]) * Bk) < 1e-15
    for k in ("d_raw", "g_mlp", "g_tab"):                     # the means divide by B: the same sums, nothing from the empty rays
        assert S.rel_max(full[k] * B, part[k] * Bk) < 1e-13, k


# ---------------------------------------------------------------- sensitivity, on the GPU test's inputs
ARMS = {"plain": dict(precision=22, full=False), "full": dict(precision=22, full=True), "full16": dict(precision=16, full=True)}
IN_PLAIN = ("step_world_x2", "d_raw_shifted", "no_pos_offset", "prev_table_grad")      # the others need an option that is off there
_cache = {}


def _arm(arm):
    """The arm's inputs, the oracle's result on them, the float32 oracle's error and the bars (computed once)."""
    if arm in _cache:
        return _cache[arm]
    from nerf_meets_mlx_amd.dataset import synthetic
    a, sh, hs = ARMS[arm], S.SHAPE, S.HASH
    imgs, poses, _, _, K = synthetic.make_dataset(sh["H"], sh["W"], sh["n_train"], seed=0, rgba=a["full"])
    res = O.hashgrid_resolutions(hs["n_levels"], hs["min_res"], hs["max_res"])
    tables = S.init_tables(hs["n_levels"], hs["log2_hashmap_size"], hs["n_features_per_level"], hs["hash_init_scale"], sh["seed"])
    occ = S.half_space_cells() if a["full"] else None
    cases = []
    for index in (0, 1):
        rays, target, bg = S.batch(imgs, poses, K, index, a["full"])
        jitter = torch.rand(sh["N_rand"], generator=torch.Generator().manual_seed(77 + index))
        offsets, rows, z, Kp = M.march(rays, jitter, occ, sh["log2_res"], S.POS_SCALE, S.POS_OFFSET, STEP, sh["march_steps"])
        cases.append(dict(offsets=offsets, rows=rows, z=z, rays=rays, target=target, background=bg if a["full"] else "white",
                          step_world=STEP, march_steps=sh["march_steps"], dist_weight=S.DIST_WEIGHT if a["full"] else None,
                          level_weights=LV.schedule(*S.LEVEL_ANNEAL, hs["n_levels"], 256) if a["full"] else None,
                          tables=tables, res=res, p_flat=S.init_mlp(sh["seed"]), pos_scale=S.POS_SCALE, pos_offset=S.POS_OFFSET,
                          emulate_bf16=a["precision"] == 16))
    case = cases[0]
    base = S.step(**case)
    f32 = S.errors(S.step(**case, dtype=torch.float32), base, case["level_weights"])
    _cache[arm] = (case, base, S.step(**cases[1])["g_tab"], f32, S.bars(a["precision"], f32))
    return _cache[arm]


@pytest.mark.parametrize("arm", list(ARMS))
def test_the_chosen_inputs_meet_the_conditions_with_the_oracle_alone(arm):
    case, base, _, f32, bars = _arm(arm)
    counts = case["offsets"][1:] - case["offsets"][:-1]
    Kp, B = int(case["offsets"][-1]), counts.numel()
    assert int((counts == 0).sum()) >= 1 and int((counts == 1).sum()) >= 1 and int((counts >= 8).sum()) >= 1
    assert 0 < Kp < B * S.SHAPE["march_steps"]
    if ARMS[arm]["full"]:
        free = M.march(case["rays"], 0.5, None, 7, S.POS_SCALE, S.POS_OFFSET, STEP, 64)[3]
        assert Kp < free, "the half-space does not cull"
        lw = case["level_weights"]
        assert any(0 < w < 1 for w in lw) and any(w == 0 for w in lw) and any(w == 1 for w in lw)
    assert float(base["raw"][:, 3].max()) < 15.0
    assert float(base["g_mlp"].norm()) > 1e-3 and float(base["g_tab"].norm()) > 1e-4, "dead network"
    print(f"[march-step oracle {arm}] K = {Kp}; float32 oracle vs float64: " + ", ".join(f"{k} {v:.1e}" for k, v in f32.items()))
    print(f"[march-step oracle {arm}] bars: " + ", ".join(f"{k} {v:.1e}" for k, v in bars.items()))


@pytest.mark.parametrize("arm,mutation", [(a, m) for a in ARMS for m in S.MUTATIONS if a != "plain" or m in IN_PLAIN])
def test_every_wrong_wiring_clears_ten_times_the_bar(arm, mutation):
    """Precision 22: a gradient quantity (g_mlp, g_tab, or one live level of g_tab) moves by >= 10 x its bar.  Precision 16, whose
    bf16 bars are 50 x wider: a checked quantity does -- the gradients where they can, else the distortion value or the float32
    compositing links evaluated at the kernel's own raw (S.given_raw; a mutation of those links leaves raw alone, so its d_raw
    there moves as the oracle's d_raw does), held to the precision-22 figures in every arm.  Halving the distortion positions can
    never move a gradient by more than half its norm, and 10 x 5e-2 is that half."""
    case, base, prev, f32, bars = _arm(arm)
    got = S.step(**case, mutate=mutation, prev_g_tab=prev)
    e = S.errors(got, base, case["level_weights"])
    margin = {k: e[k] / bars[k] for k in e if k.startswith("g_")}
    if ARMS[arm]["precision"] == 16:
        margin["dist"] = e.get("dist", 0.0) / bars.get("dist", 1.0)
        if torch.equal(got["raw"], base["raw"]):
            links = S.bars(22, f32)
            margin["d_raw|raw"] = e["d_raw"] / links["d_raw"]
            margin["loss|raw"] = e["loss"] / links["loss"]
    best = max(margin, key=margin.get)
    print(f"[march-step oracle {arm}] {mutation}: {best} moves by {margin[best]:.1f} x its bar")
    assert margin[best] >= 10.0, (mutation, best, margin[best])
