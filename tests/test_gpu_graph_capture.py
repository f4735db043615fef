"""hipGraph capture and replay of the hot path against eager launches, bit for bit.

include/nerf_hip.h promises of every entry point that its work is enqueued on `stream` and may be captured into a hipGraph.  The
law asserted here (no tolerance anywhere; `torch.equal` / `bits_equal`): a replay equals the eager call made with the same
host-side arguments on the current contents of the device buffers.  Each case captures once (tests/_capture.py: an eager
warm-up on a side stream, then one single-stream recording), then runs three rounds: new contents are written into the static
input buffers, the graph is replayed into sentinel-filled outputs, and the result is compared with an eager call on the same
contents.

  1. the ring kernels of the 8 x 256 view model at precisions 16, 22 and 32 on 7 persistent workgroups, with `nerf_mlp_pack`
     inside the graph, parameters perturbed between replays, and the pass-queue slot walked round to the captured one;
  2. one training step of the 2 x 64 hash-grid field (float32 tables, fp16 shadow; fused and unfused rows) with both Adam
     updates inside the graph, against an eager twin;
  3. the staged render chain and `nerf_render_rays_fused`, against each other and eager;
  4. `Trainer.train_step` captured after a validation render (the order in which a lazily skipped pack is missing from the
     graph), and an eager render between the recording and the first replay (a recorded pack has not run);
  5. case 2 against float64 oracle steps: the replayed training is right, not only equal to eager;
  6. what cannot be captured is refused: bias-corrected Adam, optimiser state that does not exist yet, NGPTrainer.train_step, a
     culled query's host read -- and the stream works afterwards;
  7. the first launch ever of a kernel form inside a capture, in a fresh child process (tests/_capture_child.py).
"""
import contextlib
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch

from oracle import nerf_oracle as O
from tests import _march_step_ref as S
from tests._capture import capture, capture_raises, replay
from tests._poison import PATTERNS, bits_equal, sentinel_

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS = 3
CHILD_SECONDS = 120          # import and library load take most of it (tests/test_gpu_mlp_launch.py)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"


@contextlib.contextmanager
def options(**kv):
    """nerf_set_option for the duration of a block; the previous values are restored whatever happens."""
    from nerf_meets_mlx_amd import _native as N
    lib = N.lib()
    old = {k: lib.nerf_get_option(k.encode()) for k in kv}
    try:
        for k, v in kv.items():
            N.check(lib.nerf_set_option(k.encode(), int(v)))
        yield
    finally:
        for k, v in old.items():
            N.check(lib.nerf_set_option(k.encode(), v))


def _view(precision, seed):
    from nerf_meets_mlx_amd.models.NeRF import NeRF
    arch = O.NerfArch()
    m = NeRF(channel_input=63, channel_input_views=27, is_use_view_directions=True, device=DEV, seed=seed, precision=precision)
    m.load_flat(O.flatten_params(arch, O.init_params(arch, seed)) * 1.5)
    return m


def _rays_z(B, n, seed):
    g = torch.Generator().manual_seed(seed)
    o = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=-1) * 4.0
    rays = O.pack_rays(o, -o / 4.0 + 0.25 * torch.randn(B, 3, generator=g), 2.0, 6.0)
    z = torch.sort(torch.rand(B, n, generator=g) * 4 + 2, -1).values
    return rays.to(DEV), z.to(DEV)


def _randn(shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(DEV)


def _rand(shape, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


# ------------------------------------------------------------------------------------------------ 1. the ring kernels
# Samples per pass (tests/test_gpu_pass_coverage.py): split-fp16 inference with f22_tiles 2 and split-bf16 training 128, the bf16
# ring kernels 256, fp32 128.  21 P + P / 2 is the smallest size of that file's boundary list at which each of the 7 workgroups
# runs three passes; one more row adds a partly filled 32-sample tile.
PASS = {22: 128, 16: 256, 32: 128}


@pytest.mark.parametrize("pass_queue", [1, 0])
@pytest.mark.parametrize("precision", [16, 22, 32])
def test_ring_kernels_replay_equals_eager(precision, pass_queue):
    """Three graphs of one model: inference `query`; `query(train=True)` then `backward`; and `nerf_mlp_pack` into a second image
    followed by a query from it, through the C ABI with outputs allocated before the capture.  The first two hold the model's own
    lazy pack: between replays the parameters are perturbed in place, and a graph that did not hold its pack would answer with
    the weights of capture time.  Workspaces are refilled with NaN / large bytes before every replay.  Once, 256 one-tile eager
    launches of the same entries on the same stream walk the unit's round-robin back to the captured pass-queue slot: the next
    replay finds it cleared by `leave()`."""
    from nerf_meets_mlx_amd import _native as N
    lib = N.lib()
    P = PASS[precision]
    M = 21 * P + P // 2 + 1
    assert M % 32 != 0 and (M + P - 1) // P >= 3 * 7
    m = _view(precision, seed=3)
    rays, z = _rays_z(M, 1, 1000)
    d_raw = _randn((M, 1, 4), 2000)
    tiny_rays, tiny_z = _rays_z(32, 1, 5)
    tiny_d = _randn((32, 1, 4), 6)
    image2 = torch.zeros_like(m.packed())
    raw2 = sentinel_(torch.empty(M, 1, 4, dtype=torch.float32, device=DEV))

    def pack_and_query():
        N.check(lib.nerf_mlp_pack(C.byref(m.arch), N.ptr(m.params), N.ptr(image2), N.stream()))
        N.check(lib.nerf_query_fused(C.byref(m.arch), N.ptr(image2), N.ptr(rays), N.ptr(z), M, 1, 0, N.ptr(raw2), None, N.stream()))
        return raw2

    def train():
        raw = m.query(rays, z, train=True)
        return raw, m.backward(d_raw)

    opts = dict(ring_workgroups=7, pass_queue=pass_queue)
    if precision == 22:
        opts["f22_tiles"] = 2
    with options(**opts):
        g_inf, o_inf = capture(lambda: m.query(rays, z))
        g_abi, o_abi = capture(pack_and_query)
        g_trn, o_trn = capture(train)
        scratch = [m._ws["acts"], m._ws["dz"]]
        for r in range(ROUNDS):
            nr, nz = _rays_z(M, 1, 1001 + r)
            rays.copy_(nr); z.copy_(nz); d_raw.copy_(_randn((M, 1, 4), 2001 + r))
            m.params.add_(_randn((m.n_params,), 3000 + r, 0.01))              # in place, on the device: the graphs must follow
            pat = PATTERNS[r % 2]
            got_inf = replay(g_inf, o_inf).clone()
            got_abi = replay(g_abi, o_abi).clone()
            got_raw, got_grads = (t.clone() for t in replay(g_trn, o_trn, scratch=scratch, pattern=pat))
            want_inf = m.query(rays, z)
            assert bits_equal(got_inf, want_inf), (r, "inference")
            assert bits_equal(got_abi, want_inf), (r, "pack + query through the ABI")
            want_raw = m.query(rays, z, train=True)
            want_grads = m.backward(d_raw)
            assert bits_equal(got_raw, want_raw), (r, "training forward")
            assert bits_equal(got_grads, want_grads), (r, "gradients")
            assert r == 0 or not bits_equal(got_inf, first_inf), "the rounds do not differ"
            if r == 0:
                first_inf = got_inf
                if pass_queue:
                    for _ in range(256):                     # one tile each: the round-robin of every unit returns to its start
                        m.query(tiny_rays, tiny_z)
                        m.query(tiny_rays, tiny_z, train=True)
                        m.backward(tiny_d)
                    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. / 5. the hash-grid field
# L, log2_T, F: the smallest row of NGP_CASES (tests/test_gpu_hashgrid.py) the fused 2 x 64 query takes (it needs L = 16, F = 2).
NGP = dict(n_levels=16, min_res=16, max_res=2048, n_features_per_level=2, log2_hashmap_size=19, hash_init_scale=0.5)
NGP_B, NGP_N = 65, 33
LR, BETAS, EPS = 5e-4, (0.9, 0.99), 1e-8
FIELD_ARMS = [(22, False, True), (22, False, False), (16, True, True)]          # precision, fp16 shadow, fused rows


def _field(precision, half):
    """A live field (the seed's network has sigma < 0 everywhere: DESIGN.md section 7; the alpha bias is lifted as
    tests/test_gpu_parity.py does) and its optimiser, without bias correction: a captured step bakes the correction factors."""
    from nerf_meets_mlx_amd.engine.ngp import HashNeRF
    from nerf_meets_mlx_amd.models.NeRF import Adam
    f = HashNeRF(device=DEV, seed=3, precision=precision, half_tables=half, **NGP)
    f.mlp.name = "mlp"
    p = f.mlp.params.detach().clone()
    p[10496] += 0.6
    f.mlp.load_flat(p)
    assert (f.table.half is not None) == half and f.deterministic
    return f, Adam(LR, betas=BETAS, eps=EPS, bias_correction=False, shared_state=False)


def _field_step(f, opt, rays, target, fused):
    from nerf_meets_mlx_amd import sampling
    from nerf_meets_mlx_amd.rendering import render
    z = sampling.sample_coarse(rays, NGP_N)
    raw = f.query(rays, z, train=True, fused=fused)
    loss, d_raw, _ = render.composite_mse_backward(raw, z, rays, target, True)
    g_mlp, g_tab = f.backward(d_raw, accumulate=True)         # the accumulator is zero: fresh, or cleared by the table Adam
    opt.update(f.table, g_tab.view(-1), zero_grads=True)
    opt.update(f.mlp, g_mlp)
    return {"raw": raw, "d_raw": d_raw, "loss": loss, "z": z}


def _field_batch(k):
    return _rays_z(NGP_B, 1, 400 + k)[0], _rand((NGP_B, 3), 500 + k)


def _field_state(f, opt):
    s = {"mlp": f.mlp.params, "tables": f.table.params, "accumulator": f.enc.grad}
    for key in ("mlp", "tables"):
        s[key + " m"], s[key + " v"] = opt.state[key]
    if f.table.half is not None:
        s["shadow"] = f.table.half
    return s


def _oracle_steps(precision, p0, t0, res, batches):
    """float64 training on the batches, from the oracle alone: OracleNGP.render (tests/test_gpu_parity.py) + MSE + autograd, then
    oracle.adam_step without bias correction on the network and on the tables (tests/test_gpu_march_step.py), on the device."""
    orc = O.OracleNGP(torch.zeros(1, 2, 2), res, seed=3, n_samples=NGP_N, emulate_bf16=precision == 16)
    orc.p = p0.double().to(DEV).requires_grad_(True)
    orc.tables = t0.double().to(DEV).requires_grad_(True)
    mp = [torch.zeros_like(orc.p), torch.zeros_like(orc.p)]
    mt = [torch.zeros_like(orc.tables), torch.zeros_like(orc.tables)]
    for it, (rays, target) in enumerate(batches):
        loss = O.mse(orc.render(rays.double()), target.double())
        gp, gt = torch.autograd.grad(loss, [orc.p, orc.tables])
        with torch.no_grad():
            O.adam_step(orc.p, gp, mp[0], mp[1], LR, BETAS[0], BETAS[1], EPS, False, it + 1)
            O.adam_step(orc.tables, gt, mt[0], mt[1], LR, BETAS[0], BETAS[1], EPS, False, it + 1)
    return orc.p.detach(), orc.tables.detach()


@pytest.mark.parametrize("precision,half,fused", FIELD_ARMS, ids=["p22-f32-fused", "p22-f32-rows", "p16-fp16shadow-fused"])
def test_hash_grid_training_step_replay_equals_eager_and_tracks_the_oracle(precision, half, fused):
    """Cases 2 and 5.  The graph: sample_coarse, query(train=True), composite_mse_backward, field.backward (the deterministic
    fixed-point scatter), Adam with zero_grads on the tables (it writes the fp16 shadow in the same pass), Adam on the network.
    The capture's warm-up is step 0 (it creates the moments); three replays on three further batches.  After each, parameters,
    tables, both pairs of moments, the shadow and the cleared accumulator equal those of a twin from the same seed that took the
    same steps eagerly.  (The loss word is a float-atomic sum of per-block partials -- tests/test_gpu_march_step.py -- and is
    only checked for having been written.)

    Then the four steps against the float64 oracle: relative L2 of the network's parameters and of the tables under
    tests/_march_step_ref.PROJECT[precision]["grad"] (1e-3 / 5e-2, the project's gradient figures).  Adam without bias
    correction moves an entry by about lr * 3 whatever the gradient's size, so the update is compared through the parameters it
    produces, not on its own; at precision 22 the oracle's four steps move the network by more than four times the bar (asserted),
    at precision 16 the bar bounds gross errors only."""
    a, opt_a = _field(precision, half)
    b, opt_b = _field(precision, half)
    p0, t0 = a.mlp.params.detach().clone(), a.enc.tables.detach().clone()
    batches = [_field_batch(k) for k in range(1 + ROUNDS)]
    rays, target = batches[0][0].clone(), batches[0][1].clone()
    graph, outs = capture(lambda: _field_step(a, opt_a, rays, target, fused))
    _field_step(b, opt_b, *batches[0], fused)
    for r in range(ROUNDS):
        rays.copy_(batches[1 + r][0]); target.copy_(batches[1 + r][1])
        replay(graph, outs)
        want = _field_step(b, opt_b, *batches[1 + r], fused)
        for k in ("raw", "d_raw", "z"):
            assert bits_equal(outs[k], want[k]), (r, k)
        sa, sb = _field_state(a, opt_a), _field_state(b, opt_b)
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (r, k)
        assert int(a.enc.grad.ne(0).sum()) == 0, "the table Adam left a gradient behind"
        assert float(outs["d_raw"].abs().max()) > 0, "dead network: the comparison would be 0 == 0"
    assert not torch.equal(a.mlp.params, p0) and not torch.equal(a.enc.tables, t0)
    # the eager calls after the replays see the replayed state: the bookkeeping the capture left says "stale"
    rz = _rays_z(NGP_B, NGP_N, 77)
    assert bits_equal(a.query(*rz), b.query(*rz))
    # case 5
    want_p, want_t = _oracle_steps(precision, p0, t0, a.enc.scaled_res, batches)
    bar = S.PROJECT[precision]["grad"]
    err_p, err_t = S.rel_l2(a.mlp.params, want_p), S.rel_l2(a.enc.tables, want_t)
    moved = S.rel_l2(p0, want_p)
    print(f"[capture, hash grid p{precision}] network {err_p:.1e}, tables {err_t:.1e} of the float64 oracle (bar {bar:.0e}); "
          f"the oracle's four steps move the network by {moved:.1e}")
    assert err_p < bar and err_t < bar, (err_p, err_t, bar)
    if precision == 22:
        assert moved > 4 * bar, (moved, bar)


# ------------------------------------------------------------------------------------------------ 3. staged and fused rendering
def test_staged_and_fused_rendering_replay_equal_eager_and_each_other():
    """B = 65 rays of a 16 x 16 frame generated inside the graph from a static pixel list, n = 64, N = 128 with `u` given.  One
    graph holds the staged chain (ray_gen, sample_coarse, query, composite, importance_sample, query, composite, and the MSE
    of the picture), one holds ray_gen and `nerf_render_rays_fused`.  On the keys of
    test_render_rays_fused_equals_staged_path both replays equal each other and the eager calls."""
    from nerf_meets_mlx_amd import sampling
    from nerf_meets_mlx_amd.dataset import synthetic
    from nerf_meets_mlx_amd.ops.metric import mse_loss_grad
    from nerf_meets_mlx_amd.rendering import ray, render
    H = W = 16
    B, n, Nn = 65, 64, 128
    Kc = synthetic.intrinsics(H, W)[0]
    c2w = O.pose_spherical(45.0, -30.0, 4.0)[:3, :4]
    mc, mf = _view(22, seed=5), _view(22, seed=6)
    idx = torch.randperm(H * W, generator=torch.Generator().manual_seed(1))[:B].to(DEV)
    u, target = _rand((B, Nn), 2), _rand((B, 3), 3)

    def staged():
        rays = ray.gen_rays(H, W, Kc, c2w, 2.0, 6.0, idx)
        z = sampling.sample_coarse(rays, n)
        raw = mc.query(rays, z)
        rgb_c, _, acc_c, w, _ = render.composite(raw, z, rays, 0.0, True)
        _, z_f = sampling.importance_sample(z, w, Nn, u=u)
        rgb, disp, acc, _, _ = render.composite(mf.query(rays, z_f), z_f, rays, 0.0, True, need_weights=False)
        loss, d_rgb = mse_loss_grad(rgb, target)
        return {"rgb_map": rgb, "disp_map": disp, "acc_map": acc, "rgb_coarse": rgb_c, "acc_coarse": acc_c, "z_vals": z, "weights": w,
                "d_rgb": d_rgb, "loss": loss}

    def fused():
        rays = ray.gen_rays(H, W, Kc, c2w, 2.0, 6.0, idx)
        o = render.render_rays_fused(rays, mc, mf, n, Nn, u=u, white_bkgd=True)
        return {"rgb_map": o["rgb_map"], "disp_map": o["disp_map"][:, 0], "acc_map": o["acc_map"][:, 0], "rgb_coarse": o["rgb_coarse"],
                "acc_coarse": o["acc_coarse"][:, 0], "z_vals": o["z_vals"], "weights": o["weights"][..., 0]}

    g_s, o_s = capture(staged)
    g_f, o_f = capture(fused)
    for r in range(ROUNDS):
        idx.copy_(torch.randperm(H * W, generator=torch.Generator().manual_seed(10 + r))[:B].to(DEV))
        u.copy_(_rand((B, Nn), 20 + r)); target.copy_(_rand((B, 3), 30 + r))
        got_s = {k: v.clone() for k, v in replay(g_s, o_s).items()}
        got_f = {k: v.clone() for k, v in replay(g_f, o_f).items()}
        want_s, want_f = staged(), fused()
        for k in got_f:
            assert bits_equal(got_s[k], want_s[k]), (r, "staged", k)
            assert bits_equal(got_f[k], want_f[k]), (r, "fused", k)
            assert bits_equal(got_s[k], got_f[k]), (r, "staged against fused", k)
        assert bits_equal(got_s["d_rgb"], want_s["d_rgb"]), r
        assert r == 0 or not bits_equal(got_s["rgb_map"], first), "the rounds do not differ"
        first = got_s["rgb_map"]


# ------------------------------------------------------------------------------------------------ 4. the order that bites
def _trainer(precision):
    from nerf_meets_mlx_amd.dataset import synthetic
    from nerf_meets_mlx_amd.engine.trainer import Trainer
    imgs, poses, _, _, K = synthetic.make_dataset(16, 16, 2, seed=0, device=DEV)
    return Trainer(imgs, poses, K, N_rand=64, seed=4, device=DEV, precision=precision)


def _trainer_batches(tr, count):
    out = []
    for k in range(count):
        idx = torch.randperm(256, generator=torch.Generator().manual_seed(40 + k))[:64].to(DEV)
        rays, target = tr.sample_batch(pixel_idx=idx, img_i=k % 2)
        out.append((rays.clone(), target.clone(), _rand((64, 128), 50 + k)))
    return out


def _trainer_state(tr):
    m, v = tr._opt.state["shared"]
    return {"coarse": tr.coarse.params, "fine": tr._fine.params, "m": m, "v": v}


def _assert_same_training_state(a, b, tag):
    sa, sb = _trainer_state(a), _trainer_state(b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), (tag, k, int((sa[k] != sb[k]).sum()), sa[k].numel())


@pytest.mark.parametrize("precision", [16, 22])
def test_train_step_captured_after_a_validation_render(precision):
    """The order an ordinary training script makes: a training step (the capture's eager warm-up), a render of a few rays,
    then the recording of `train_step(rays, target, u)`, three replays, a render.  The render packs both networks and leaves
    their images current, so a pack that is skipped when the image is current is missing from the graph: every replay would run
    the fine network (and, without one, the coarse) on the weights of capture time while the captured Adam moves the float32
    masters.  NeRF.packed() therefore always records its pack under capture.

    The twin is an eager trainer from the same seed making the same calls, with `it` set to the value it had at the recording
    before each step: the schedule's learning rate is a host float passed by value, which the graph bakes (include/nerf_hip.h).
    After each replay the parameters of both networks and the shared moments are equal bit for bit, and so is a render after
    the last."""
    a, b = _trainer(precision), _trainer(precision)
    batches = _trainer_batches(a, 1 + ROUNDS)
    rays, target, u = (t.clone() for t in batches[0])
    few, u_few = batches[0][0][:5].clone(), batches[0][2][:5].clone()
    at = {}

    def validate():
        at["render"] = a.render_rays(few, u=u_few).clone()
        at["it"] = a.it

    graph, outs = capture(lambda: a.train_step(rays, target, u), before_record=validate)
    b.train_step(*batches[0])
    assert torch.equal(at["render"], b.render_rays(few, u=u_few))
    assert at["it"] == b.it == 1
    _assert_same_training_state(a, b, "before the first replay")
    for r in range(ROUNDS):
        for dst, src in zip((rays, target, u), batches[1 + r]):
            dst.copy_(src)
        replay(graph, outs)
        b.it = at["it"]
        b.train_step(*batches[1 + r])
        _assert_same_training_state(a, b, f"replay {r}")
    assert torch.equal(a.render_rays(few, u=u_few), b.render_rays(few, u=u_few))


@pytest.mark.parametrize("precision", [16, 22])
def test_eager_render_between_the_recording_and_the_first_replay(precision):
    """Recording, one eager render, first replay.  A pack recorded into the graph has not run: the bookkeeping must go on saying
    "stale", so that the eager render packs for itself instead of reading an image nobody wrote.  That render leaves the images
    current; the replay behind it moves the parameters without the host knowing, so the render after the replay has to pack
    again: a model whose optimiser step lives in a graph packs at every eager use.  The twin and the baked learning rate are
    those of the test above."""
    a, b = _trainer(precision), _trainer(precision)
    batches = _trainer_batches(a, 2)
    rays, target, u = (t.clone() for t in batches[0])
    few, u_few = batches[0][0][:5].clone(), batches[0][2][:5].clone()
    graph, outs = capture(lambda: a.train_step(rays, target, u))
    it = a.it - 1
    b.train_step(*batches[0])
    assert it == b.it == 1
    assert torch.equal(a.render_rays(few, u=u_few), b.render_rays(few, u=u_few))
    for dst, src in zip((rays, target, u), batches[1]):
        dst.copy_(src)
    replay(graph, outs)
    b.train_step(*batches[1])
    _assert_same_training_state(a, b, "first replay")
    assert torch.equal(a.render_rays(few, u=u_few), b.render_rays(few, u=u_few))


def test_a_pack_recorded_but_not_run_is_not_trusted():
    """The same rule on one model: parameters edited, an inference query recorded (its pack is in the graph and has not run), then
    an eager query before any replay: it equals the query of a twin that was never captured."""
    a, b = _view(22, seed=8), _view(22, seed=8)
    rays, z = _rays_z(65, 3, 9)
    a.query(rays, z); b.query(rays, z)
    graph = torch.cuda.CUDAGraph()
    delta = _randn((a.n_params,), 11, 0.01)
    a.params.add_(delta); b.params.add_(delta)
    with torch.cuda.graph(graph):
        out = a.query(rays, z)
    torch.cuda.synchronize()
    want = b.query(rays, z)
    assert bits_equal(a.query(rays, z), want)
    assert bits_equal(replay(graph, out), want)


# ------------------------------------------------------------------------------------------------ 6. refusals
def _probe():
    """A small eager launch and its result: made before and after a refused capture, the two must agree."""
    from nerf_meets_mlx_amd import sampling
    z = sampling.sample_coarse(_rays_z(7, 1, 1)[0], 9)
    torch.cuda.synchronize()
    return z


def _flat(n=1000):
    from nerf_meets_mlx_amd.engine.ngp import _Flat
    return _Flat(_randn((n,), 1), _randn((n,), 2))


@pytest.mark.parametrize("method", ["update", "update_spans"])
def test_adam_refuses_what_a_replay_would_get_wrong(method):
    """Under capture: bias correction (factors computed on the host from the step count, by value) and a key without state (the
    zeroed moments would be cleared by every replay) raise ValueError before anything is recorded or counted; with the state in
    place and no bias correction the same call is captured, and three replays equal three eager updates."""
    from nerf_meets_mlx_amd.models.NeRF import Adam
    before = _probe()

    def call(opt, model):
        if method == "update":
            opt.update(model)
        else:
            opt.update_spans(model, [(0, 600, model.grads[0:600]), (600, 1000, model.grads[600:1000])])

    model = _flat()
    kept = model.params.clone()
    corrected = Adam(1e-2, bias_correction=True, shared_state=False)
    call(corrected, model)                                   # eagerly it works, and creates the state
    err = capture_raises(lambda: call(corrected, model))
    assert isinstance(err, ValueError) and "bias_correction" in str(err), repr(err)
    assert corrected.step_count == {"tables": 1}
    fresh, model2 = Adam(1e-2, shared_state=False), _flat()
    err = capture_raises(lambda: call(fresh, model2))
    assert isinstance(err, ValueError) and "state" in str(err), repr(err)
    assert fresh.state == {} and fresh.step_count == {} and torch.equal(model2.params, kept)
    assert torch.equal(_probe(), before)
    twin, opt_t = _flat(), Adam(1e-2, shared_state=False)
    graph, _ = capture(lambda: call(fresh, model2))          # the warm-up creates the state; the recording is accepted
    call(opt_t, twin)
    for r in range(ROUNDS):
        g = _randn((1000,), 60 + r)
        model2.grads.copy_(g); twin.grads.copy_(g)
        replay(graph, None)
        call(opt_t, twin)
        assert torch.equal(model2.params, twin.params), r
        for x, y in zip(fresh.state["tables"], opt_t.state["tables"]):
            assert torch.equal(x, y), r


SMALL_NGP = dict(n_levels=16, min_res=4, max_res=128, n_features_per_level=2, log2_hashmap_size=12, hash_init_scale=0.5)


def _ngp_trainer(**kw):
    from nerf_meets_mlx_amd.dataset import synthetic
    from nerf_meets_mlx_amd.engine.ngp import NGPTrainer
    imgs, poses, _, _, K = synthetic.make_dataset(16, 16, 2, seed=0, device=DEV)
    return NGPTrainer(imgs, poses, K, N_rand=64, n_depth_samples=32, seed=0, device=DEV, **SMALL_NGP, **kw)


def test_ngp_trainer_train_step_refuses_capture():
    """NGPTrainer's Adam is bias-corrected: its train_step raises ValueError under capture, and trains on eagerly afterwards as
    a twin that was never captured does."""
    before = _probe()
    a, b = _ngp_trainer(), _ngp_trainer()
    rays, target = a.sample_batch()
    a.train_step(rays, target); b.train_step(rays, target)
    err = capture_raises(lambda: a.train_step(rays, target))
    assert isinstance(err, ValueError) and "bias_correction" in str(err), repr(err)
    assert a.it == b.it == 1
    assert torch.equal(_probe(), before)
    a.train_step(rays, target); b.train_step(rays, target)
    assert torch.equal(a.field.mlp.params, b.field.mlp.params) and torch.equal(a.field.table.params, b.field.table.params)


def test_a_culled_step_fails_on_its_host_read_under_capture():
    """With an occupancy grid, past the warm-up, the training query reads its sample count back to the host: under capture that
    read fails (RuntimeError from the runtime) before Adam is reached, the capture is ended, nothing is replayed, and the stream
    is usable."""
    from nerf_meets_mlx_amd.engine.occupancy import WARMUP
    before = _probe()
    tr = _ngp_trainer(occupancy_grid=True)
    rays, target = tr.sample_batch()
    tr.it = WARMUP
    tr.train_step(rays, target)
    tr.it = WARMUP
    err = capture_raises(lambda: tr.train_step(rays, target))
    assert isinstance(err, RuntimeError) and not isinstance(err, ValueError), repr(err)
    assert tr.it == WARMUP
    assert torch.equal(_probe(), before)


def test_the_stream_launches_and_matches_eager_after_the_refusals():
    m = _view(22, seed=2)
    rays, z = _rays_z(65, 3, 4)
    graph, out = capture(lambda: m.query(rays, z))
    assert bits_equal(replay(graph, out).clone(), m.query(rays, z))


# ------------------------------------------------------------------------------------------------ 7. opt-in group under capture
def _child(mode):
    cmd = ["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, os.path.join(ROOT, "tests", "_capture_child.py"), mode]
    out = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0, f"child {mode}: exit {out.returncode}\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}"
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


def test_first_launch_of_a_kernel_form_inside_a_capture():
    """csrc/launch.h: a form's first launch inside a capture meets nothing it cannot do there.  In a fresh process the rows form
    of the split-fp16 inference kernels is launched eagerly; the first launches ever of the 32- and 48-samples-per-wave forms
    (same translation unit, same LDS opt-in) are recorded and replayed.  Their outputs equal those of a second child that launched
    all three eagerly."""
    a = _child("capture")              # (an exit code other than 0 fails here: the second child is not started)
    b = _child("eager")
    assert a["error"] == "" and b["error"] == "", (a["error"], b["error"])
    assert set(a["digests"]) == set(b["digests"]) == {"rows", "f22_tiles=2", "f22_tiles=3"}
    assert a["digests"] == b["digests"], (a["digests"], b["digests"])
    assert a["digests"]["f22_tiles=2"] != a["digests"]["rows"]
