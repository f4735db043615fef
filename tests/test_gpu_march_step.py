"""The march-mode training step as NGPTrainer wires it -- grid update, ragged march, packed fused query, packed compositing with
trunc_exp density (over a per-ray background against an RGBA target, with the distortion regulariser), 2 x 64 backward with input
gradients, level-weighted scatter in level groups, two Adam launches -- against the end-to-end float64 oracle of
tests/_march_step_ref.py.  Every link has its own bit-exact or float64 test; this file tests the chain.

Arms: plain (precision 22, white, iteration 0: no culling), full (random backgrounds, RGBA, distortion, level_anneal at iteration
WARMUP: the bitfield culls, level weights 1, fractional and 0), full16 (the same at precision 16 with half tables, against the
bf16-emulating oracle), float-scatter (plain with deterministic=False).

Inputs: tests/_march_step_ref.batch -- 64 seeded rays of a 4 x 16 x 16 synthetic set, one edited to meet nothing and one to take
exactly one step.  The step's packed samples are replayed by the test: the jitter of counter stream 4 and the grid's own march
(the march reads the bitfield, never the tables).  The culled arms get their bitfield through the grid's own state: a half-space
of huge densities is written, the threshold cap raised above any density the field can add, and the grid's finalize run, so
that the update the step itself performs at iteration WARMUP (256 is a multiple of UPDATE_EVERY) merges the field's densities
and finalizes to the same half-space -- which the test checks by marching the same rays with tests/_march_ref.march.

Bars (DESIGN.md "March-mode step against the end-to-end oracle"): the project's figures for the fixed-grid path -- loss 1e-3,
raw 1e-4 of its max, gradients 1e-3 rel-L2 at precision 22 (tests/test_gpu_round5.py); loss 2e-2, gradients 5e-2 at precision 16
(tests/test_gpu_parity.py), raw 1e-2 (the smoke run's figure); six-step tracking 2e-2 / 0.25.  d_raw, the distortion value and
the per-level table gradients take the larger of the neighbouring figure and 8 x the float32 oracle's own error against float64
on the same inputs (computed here, from the oracle alone).  The compositing and loss links are float32 kernels whatever the
network's precision: evaluated at the kernel's own raw they are held to the precision-22 figures in every arm.
tests/test_march_step_ref_host.py shows that these bars reject every wrong wiring it lists by a factor of 10 or more.
"""
import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests import _hashgrid_ref as R
from tests import _levels_ref as LV
from tests import _march_ref as M
from tests import _march_step_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
SH, HS = S.SHAPE, S.HASH
STEP = M.step_world(SH["march_steps"], SH["bound"])
RES = O.hashgrid_resolutions(HS["n_levels"], HS["min_res"], HS["max_res"])
T, F, L = 1 << HS["log2_hashmap_size"], HS["n_features_per_level"], HS["n_levels"]
ARMS = {"plain": dict(precision=22, full=False, deterministic=True), "full": dict(precision=22, full=True, deterministic=True),
        "full16": dict(precision=16, full=True, deterministic=True), "float-scatter": dict(precision=22, full=False, deterministic=False)}
BETAS, EPS = (0.9, 0.99), 1e-8
_data = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"


def _dataset(full):
    if full not in _data:
        from nerf_meets_mlx_amd.dataset import synthetic
        imgs, poses, _, _, K = synthetic.make_dataset(SH["H"], SH["W"], SH["n_train"], seed=0, rgba=full)
        _data[full] = (imgs, poses, K)
    return _data[full]


def _batch(arm, index):
    rays, target, bg = S.batch(*_dataset(ARMS[arm]["full"]), index, ARMS[arm]["full"])
    return rays.to(DEV), target.to(DEV), None if bg is None else bg.to(DEV)


def _trainer(arm):
    from nerf_meets_mlx_amd.engine.ngp import NGPTrainer
    from nerf_meets_mlx_amd.engine.occupancy import LOG2_RES, UPDATE_EVERY, WARMUP
    a = ARMS[arm]
    imgs, poses, K = _dataset(a["full"])
    kw = dict(HS, deterministic=a["deterministic"])
    if a["precision"] == 16:
        kw["half_tables"] = True
    tr = NGPTrainer(imgs.to(DEV), poses, K, N_rand=SH["N_rand"], seed=SH["seed"], device=DEV, precision=a["precision"],
                    occupancy_grid=True, march_steps=SH["march_steps"], distortion_weight=S.DIST_WEIGHT if a["full"] else None,
                    random_background=a["full"], level_anneal=S.LEVEL_ANNEAL if a["full"] else None, **kw)
    assert tr.grid.step_world == STEP and list(tr.field.enc.scaled_res) == RES and LOG2_RES == SH["log2_res"]
    assert (tr.field.pos_scale, tr.field.pos_offset) == (S.POS_SCALE, S.POS_OFFSET)
    assert torch.equal(tr.field.mlp.params.cpu(), S.init_mlp(SH["seed"]))
    assert torch.equal(tr.field.enc.tables.cpu(), S.init_tables(L, HS["log2_hashmap_size"], F, HS["hash_init_scale"], SH["seed"]))
    assert (tr.field.table.half is not None) == (a["precision"] == 16)
    if a["full"]:                                            # a run that has reached iteration WARMUP, with a hand-made grid
        assert WARMUP % UPDATE_EVERY == 0
        tr.it = WARMUP
        tr._opt.step_count = {"mlp": WARMUP, "tables": WARMUP}
        tr.grid.thr_cap = 1e3
        tr.grid.density.copy_(torch.where(S.half_space_cells(), 1e6, 0.0).float())
        tr.grid._finalize()
        tr.grid.updates = WARMUP // UPDATE_EVERY
    return tr


def _level_weights(arm, it):
    return [float(w) for w in LV.schedule(*S.LEVEL_ANNEAL, L, it)] if ARMS[arm]["full"] else None


def _replay(tr, rays, it):
    """(offsets, rows, z, K), cloned: the packed samples of the step at iteration `it` on the grid as it stands."""
    from nerf_meets_mlx_amd import parallel
    from nerf_meets_mlx_amd.engine.occupancy import WARMUP
    g = torch.Generator(device=DEV)
    g.manual_seed(parallel.counter_seed(tr.seed, tr.rank, 4, it))
    jitter = torch.rand(rays.shape[0], dtype=torch.float32, device=DEV, generator=g)
    offsets, rows, z, K = tr.grid.march(rays, jitter, use_bits=it >= WARMUP)
    return offsets.clone(), rows.clone(), z.clone(), K, jitter


def _check_conditions(arm, tr, rays, offsets, rows, z, K, jitter, it):
    """The conditions on the step's samples, and -- the oracle alone -- that they are tests/_march_ref.march's."""
    B = rays.shape[0]
    counts = (offsets[1:] - offsets[:-1]).cpu()
    assert int((counts == 0).sum()) >= 1 and int((counts == 1).sum()) >= 1 and int((counts >= 8).sum()) >= 1
    assert 0 < K < B * SH["march_steps"] and K % 16 != 0, K
    occ = S.half_space_cells() if ARMS[arm]["full"] else None
    wo, wr, wz, wK = M.march(rays.cpu(), jitter.cpu(), occ, SH["log2_res"], S.POS_SCALE, S.POS_OFFSET, STEP, SH["march_steps"])
    assert wK == K and torch.equal(wo, offsets.cpu()) and torch.equal(wz, z.cpu()) and torch.equal(wr, rows.cpu())
    if ARMS[arm]["full"]:
        free = M.march(rays.cpu(), jitter.cpu(), None, SH["log2_res"], S.POS_SCALE, S.POS_OFFSET, STEP, SH["march_steps"])[3]
        assert K < free, "the bitfield does not cull"
        lw = _level_weights(arm, it)
        assert tuple(tr.field.level_weights) == tuple(lw)
        assert any(0 < w < 1 for w in lw) and any(w == 0 for w in lw) and any(w == 1 for w in lw)


def _gradients(tr, rays, target, bg, want_dx=False):
    """Forward and gradients of one step on `tr`, no update: the trainer's own pieces in train_step's order.  Everything on the
    CPU, with the step's packed samples and the kernel's ReLU decisions."""
    from nerf_meets_mlx_amd.models.NeRF import debug_layer
    it = tr.it
    tr._apply_level_weights()
    loss, d_raw, dist = tr._march_step_forward(rays, target, bg)
    used = tuple(t.clone() for t in tr._field._rz)
    d_x = tr._field.mlp.backward(d_raw, need_input_grad=True)[1].cpu().clone() if want_dx else None
    g_mlp, acc = tr._field.backward(d_raw, accumulate=False)
    out = {"loss": loss.cpu()[0], "dist": dist.cpu()[0] if dist is not None else torch.zeros(()), "d_raw": d_raw.cpu().clone(),
           "g_mlp": g_mlp.cpu().clone(), "acc": acc.cpu().clone(), "g_tab": tr._field.table_grad().cpu().clone(), "d_x": d_x, "it": it}
    offsets, rows, z, K, jitter = _replay(tr, rays, it)
    assert K == tr.last_march[1] and torch.equal(rows, used[0]) and torch.equal(z, used[1].reshape(-1)), "the replay is not the step's march"
    out["raw"] = tr._field.query_packed(rows, z, train=True).reshape(-1, 4).cpu().clone()
    out["masks"] = {n: debug_layer(tr._field.mlp, "acts", l).cpu() > 0 for n, l in S.MASK_LAYERS}
    out.update(offsets=offsets.cpu(), rows=rows.cpu(), z=z.cpu(), K=K, jitter=jitter)
    return out


def _oracle_args(arm, got, rays, target, bg, tables, p_flat, it):
    a = ARMS[arm]
    return dict(offsets=got["offsets"], rows=got["rows"], z=got["z"], rays=rays.cpu(), target=target.cpu(),
                background=bg.cpu() if a["full"] else "white", step_world=STEP, march_steps=SH["march_steps"],
                dist_weight=S.DIST_WEIGHT if a["full"] else None, level_weights=_level_weights(arm, it), tables=tables, res=RES,
                p_flat=p_flat, pos_scale=S.POS_SCALE, pos_offset=S.POS_OFFSET, emulate_bf16=a["precision"] == 16)


@pytest.mark.parametrize("arm", list(ARMS))
def test_forward_and_gradients_of_one_step_match_the_oracle(arm):
    """(a): loss, distortion, raw, d_raw, g_mlp and g_tab (all levels, and every level with a non-zero weight) of one step; exact
    zeros in the levels with weight 0 and in the entries no sample touches; live gradients.

    Measured on the MI355X (error / bar): see DESIGN.md "March-mode step against the end-to-end oracle"."""
    a = ARMS[arm]
    tr = _trainer(arm)
    rays, target, bg = _batch(arm, 0)
    tables, p_flat = tr.field.enc.tables.cpu().clone(), tr.field.mlp.params.cpu().clone()
    got = _gradients(tr, rays, target, bg)
    it = got["it"]
    _check_conditions(arm, tr, rays, got["offsets"].to(DEV), got["rows"].to(DEV), got["z"].to(DEV), got["K"], got["jitter"], it)
    args = _oracle_args(arm, got, rays, target, bg, tables, p_flat, it)
    want = S.step(**args, masks=got["masks"])
    lw = args["level_weights"]
    f32 = S.errors(S.step(**args, masks=got["masks"], dtype=torch.float32), want, lw)
    bars, err = S.bars(a["precision"], f32), S.errors(got, want, lw)
    links, at_raw = S.bars(22, f32), S.given_raw(got["raw"], args["offsets"], args["z"], args["rays"], args["target"],
                                                 args["background"], STEP, SH["march_steps"], args["dist_weight"])
    err_links = {"loss|raw": S.rel_abs(got["loss"], at_raw["loss"]), "d_raw|raw": S.rel_l2(got["d_raw"], at_raw["d_raw"])}
    bar_links = {"loss|raw": links["loss"], "d_raw|raw": links["d_raw"]}
    if a["full"]:
        err_links["dist|raw"], bar_links["dist|raw"] = S.rel_abs(got["dist"], at_raw["dist"]), links["dist"]
    print(f"[march step {arm}] K = {got['K']}, it = {it}; error (bar): " +
          ", ".join(f"{k} {v:.1e} ({bars[k]:.0e})" for k, v in err.items()) + "; " +
          ", ".join(f"{k} {v:.1e} ({bar_links[k]:.0e})" for k, v in err_links.items()) +
          f"; float32 oracle: d_raw {f32['d_raw']:.1e}" + (f", dist {f32['dist']:.1e}" if "dist" in f32 else "") +
          f", worst level {max(v for k, v in f32.items() if k.startswith('g_tab_l')):.1e}")
    assert float(want["raw"][:, 3].max()) < 15.0
    assert float(want["g_mlp"].norm()) > 1e-3 and float(want["g_tab"].norm()) > 1e-4, "dead network: the comparison would be 0 == 0"
    assert float(got["g_mlp"].norm()) > 1e-3 and float(got["g_tab"].norm()) > 1e-4
    for k, v in err.items():
        assert v < bars[k], (k, v, bars[k])
    for k, v in err_links.items():
        assert v < bar_links[k], (k, v, bar_links[k])
    # exact zeros: levels with weight 0, and entries no sample's corner hashes to (the kernel's float32 positions, bit for bit)
    p = R.points(got["rows"].numpy(), got["z"].numpy(), 1, S.POS_SCALE, S.POS_OFFSET)
    hit = np.zeros((L, T), bool)
    for l in S.live_levels(lw, L):
        hit[l, R.corners(p, RES[l], T)[0].reshape(-1)] = True
    assert (~hit).any() and hit.any()
    cold = torch.from_numpy(~hit)
    assert bool((got["acc"][cold] == 0).all()) and bool((want["g_tab"][cold] == 0).all())
    if a["full"]:
        dead = [l for l in range(L) if l not in S.live_levels(lw, L)]
        assert dead and bool((got["acc"][dead] == 0).all())


def _state(tr):
    f, o = tr._field, tr._opt
    zeros = lambda t: [torch.zeros_like(t), torch.zeros_like(t)]
    m = {k: [s.cpu().numpy().copy() for s in o.state.get(k, zeros(buf.params))] for k, buf in (("mlp", f.mlp), ("tables", f.table))}
    return {"mlp": f.mlp.params.cpu().numpy().copy(), "tables": f.table.params.cpu().numpy().copy(), "moments": m}


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def _check_float_sum(g_est, slack, p, d_x):
    """The table gradient a float-atomic scatter accumulated, recovered to within `slack`, against the exact sum of its addends:
    the bound of tests/test_gpu_hashgrid.py::test_float_scatter_is_within_the_summation_bound, (k + 1) 2^-24 sum |a| + k 2^-126."""
    idx, val = R.addends(p, d_x, RES, T, F, L)
    s, sa, k = R.scatter_f64(idx, val, L * T * F)
    bound = (k + 1) * 2.0 ** -24 * sa + k * 2.0 ** -126
    bad = np.flatnonzero(np.abs(g_est.astype(np.float64) - s) > bound + slack)
    assert len(bad) == 0, (len(bad), g_est[bad[:4]], s[bad[:4]], bound[bad[:4]])


@pytest.mark.parametrize("arm", list(ARMS))
def test_two_steps_are_adam_on_each_batch_s_own_gradient(arm):
    """(b): two train_steps on two batches.  A twin in the identical state gives each step's gradients as in (a); afterwards the
    parameters, tables, both pairs of moments and the fp16 shadow are tests/_hashgrid_ref.adam_ex of those gradients bit for bit
    (lr = lrate 0.1^(it / (lrate_decay 1000)), betas (0.9, 0.99), bias correction at step it + 1, grad_scale 1), the accumulator
    is zero, `it` advanced -- so the second step's gradient is its own batch's alone.  float-scatter: the MLP side bit for bit;
    on the table side the first moments hold (1 - beta1) g: the gradient recovered from them lies within the float scatter's
    summation bound of the exact sum of the batch's addends, and the tables follow from the stored moments bit for bit."""
    a = ARMS[arm]
    tr, twin = _trainer(arm), _trainer(arm)
    b1 = np.float32(BETAS[0])
    for index in (0, 1):
        rays, target, bg = _batch(arm, index)
        before, it = _state(tr), tr.it
        g = _gradients(twin, rays, target, bg, want_dx=not a["deterministic"])
        assert g["it"] == it
        out = tr.train_step(rays, target, background=bg)
        after = _state(tr)
        assert tr.it == it + 1 and twin.it == it
        # (the two reported scalars are float-atomic sums of per-block partials: the same to the order of 16 additions, not bitwise)
        assert abs(float(out["loss_coarse"]) - float(g["loss"])) <= 2.0 ** -20 * float(g["loss"]), "the twin's forward is not the step's"
        if a["full"]:
            assert abs(float(out["loss_distortion"]) - float(g["dist"])) <= 2.0 ** -20 * float(g["dist"])
        lr = tr.lrate * (0.1 ** (it / (tr.lrate_decay * 1000)))
        c1, c2 = R.bias_factors(BETAS[0], BETAS[1], True, it + 1)
        assert tr._opt.step_count == {"mlp": it + 1, "tables": it + 1}
        for key, grad, fixed in (("mlp", g["g_mlp"].numpy(), False), ("tables", g["acc"].numpy().reshape(-1), True)):
            m0, v0 = before["moments"][key]
            m1, v1 = after["moments"][key]
            if key == "tables" and not a["deterministic"]:
                c = np.float32(1.0) - b1
                est = (m1.astype(np.float64) - (b1 * m0).astype(np.float64)) / float(c)
                slack = 2.0 ** -22 * (np.abs(m0) + np.abs(m1)).astype(np.float64) / float(c)
                _check_float_sum(est, slack, R.points(g["rows"].numpy(), g["z"].numpy(), 1, S.POS_SCALE, S.POS_OFFSET), g["d_x"].numpy())
                lr32, eps32 = np.float32(lr), np.float32(EPS)
                want_p = (before[key] - lr32 * (m1 * c1) / (np.sqrt(v1 * c2) + eps32)).astype(np.float32)
                assert np.array_equal(_bits(after[key]), _bits(want_p)), "tables do not follow from the stored moments"
                continue
            wp, wm, wv = R.adam_ex(before[key], grad, m0, v0, lr, BETAS[0], BETAS[1], EPS, c1, c2, 1.0, fixed)
            for name, have, want in (("p", after[key], wp), ("m", m1, wm), ("v", v1, wv)):
                bad = np.flatnonzero(_bits(have) != _bits(want))
                assert len(bad) == 0, (key, name, index, len(bad), have[bad[:4]], want[bad[:4]])
        assert int(tr._field.enc.grad.ne(0).sum()) == 0, "the table Adam left a gradient behind"
        assert not np.array_equal(after["tables"], before["tables"]) and not np.array_equal(after["mlp"], before["mlp"])
        if tr._field.table.half is not None:
            assert torch.equal(tr._field.table.half.cpu(), torch.from_numpy(after["tables"]).half())
            assert tr._field.table._half_version == tr._field.table.params._version, "the shadow Adam wrote counts as stale"
        twin.load_state_dict(tr.state_dict())
        assert twin.it == tr.it and torch.equal(twin.grid.bits, tr.grid.bits)


@pytest.mark.parametrize("arm", list(ARMS))
def test_six_steps_track_the_oracle_loop(arm):
    """(c): six train_steps against six oracle steps (oracle.adam_step, bias-corrected at step it + 1, the same schedule) on the
    same batches and the same replayed samples: the losses -- and in the full arms the distortion values -- track step by step."""
    a = ARMS[arm]
    tr = _trainer(arm)
    tables = tr.field.enc.tables.cpu().double().clone()
    p_flat = tr.field.mlp.params.cpu().double().clone()
    mt, mp = [torch.zeros_like(tables), torch.zeros_like(tables)], [torch.zeros_like(p_flat), torch.zeros_like(p_flat)]
    track = S.PROJECT[a["precision"]]["track"]
    hip, ora, hip_d, ora_d = [], [], [], []
    for n in range(6):
        rays, target, bg = _batch(arm, 10 + n)
        it = tr.it
        out = tr.train_step(rays, target, background=bg)
        offsets, rows, z, K, _ = _replay(tr, rays, it)
        assert K == tr.last_march[1]
        got = {"offsets": offsets.cpu(), "rows": rows.cpu(), "z": z.cpu()}
        want = S.step(**_oracle_args(arm, got, rays, target, bg, tables, p_flat, it))
        lr = O.lr_schedule(tr.lrate, tr.lrate_decay, it)
        O.adam_step(p_flat, want["g_mlp"], mp[0], mp[1], lr, BETAS[0], BETAS[1], EPS, True, it + 1)
        O.adam_step(tables, want["g_tab"], mt[0], mt[1], lr, BETAS[0], BETAS[1], EPS, True, it + 1)
        hip.append(float(out["loss_coarse"])); ora.append(float(want["loss"]))
        if a["full"]:
            hip_d.append(float(out["loss_distortion"])); ora_d.append(float(want["dist"]))
    print(f"[march step {arm}] six steps: loss {['%.5f' % v for v in hip]} vs {['%.5f' % v for v in ora]}" +
          (f"; distortion {['%.5f' % v for v in hip_d]} vs {['%.5f' % v for v in ora_d]}" if a["full"] else "") +
          f"; worst {max(abs(x - y) / y for x, y in zip(hip + hip_d, ora + ora_d)):.1e} (bar {track:.0e})")
    for x, y in zip(hip + hip_d, ora + ora_d):
        assert abs(x - y) < track * y, (hip, ora, hip_d, ora_d)
    assert tr.it == (256 if a["full"] else 0) + 6
