"""Early ray termination of the march (engine/occupancy.py OccupancyGrid.render_ert, csrc/occupancy.hip nerf_ert_march_*,
csrc/composite_packed.hip nerf_ert_fold / _finish) on the GPU: at eps = 0 against the one-shot march and packed compositing, the
resumed march and the fold alone against the references, the error bound at eps > 0, schedule independence, poisoned buffers,
and the trainer (training untouched, held-out frame within eps, aux outputs in every NGP mode)."""
import numpy as np
import pytest
import torch

from tests import _ert_ref as E
from tests import _march_ref as M
from tests import _occupancy_ref as O
from tests._poison import bits_equal, sentinel_, unwritten
from tests.test_gpu_march import SENT64, _field, _grid, _rays

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"


def _random_bits(g, p, seed):
    from nerf_meets_mlx_amd.engine.occupancy import RES
    occ = torch.rand(RES ** 3, generator=torch.Generator().manual_seed(seed)) < p
    g.bits.copy_(O.pack(occ.to(DEV)))
    return occ


def _one_shot(g, field, rays, jitter, use_bits, white):
    from nerf_meets_mlx_amd.rendering import render
    offs, rows, z, K = g.march(rays, jitter, use_bits=use_bits)
    raw = field.query_packed(rows, z)
    rgb, acc, depth = render.composite_packed(raw, z, offs, rays.shape[0], g.step_world, white)
    return rgb, acc, depth, (offs[1:] - offs[:-1]).clone()


class _Dense:
    """The field with its sigma output raised by `bias` (the output layer's sigma bias): a field dense enough that rays saturate."""

    def __init__(self, field, bias):
        self.field, self.bias = field, bias

    def query_packed(self, rows, z):
        raw = self.field.query_packed(rows, z).clone()
        raw[..., 3] += self.bias
        return raw


# ------------------------------------------------------------------------------------------------ 1: eps = 0 is the one-shot render
@pytest.mark.parametrize("steps", [1, 7, 256, 1024])
@pytest.mark.parametrize("use_bits", [True, False])
def test_eps_zero_matches_the_one_shot_march(steps, use_bits):
    f = _field()
    g = _grid(f, steps)
    _random_bits(g, 0.3, 7)
    rays = _rays(512, 5)
    jit_rays = torch.rand(512, generator=torch.Generator().manual_seed(12)).float().to(DEV)
    for jitter in (0.5, jit_rays):
        for white in (False, True):
            w_rgb, w_acc, w_depth, w_n = _one_shot(g, f, rays, jitter, use_bits, white)
            o = g.render_ert(f, rays, jitter, 0.0, white, use_bits=use_bits)
            assert torch.equal(o["samples"].long(), w_n), (steps, use_bits)
            assert float((o["rgb"] - w_rgb).abs().max()) <= 2e-6
            assert float((o["acc"] - w_acc).abs().max()) <= 2e-6
            assert float((o["depth"] - w_depth).abs().max()) <= 1e-5
            assert bool(torch.isfinite(o["rgb"]).all())
            if steps > 1:
                assert int(w_n.sum()) > 0


# ------------------------------------------------------------------------------------------------ 2: the resumed march alone
@pytest.mark.parametrize("steps,m", [(64, 1), (64, 5), (1024, 7), (1024, 64)])
def test_resumed_march_matches_the_reference(steps, m):
    from nerf_meets_mlx_amd.engine.occupancy import LOG2_RES
    f = _field()
    g = _grid(f, steps)
    occ = _random_bits(g, 0.4, 8)
    B = 512
    rays = _rays(B, 6)
    keep, zc = E.march_keep(rays.cpu(), 0.5, occ, LOG2_RES, g.pos_scale, g.pos_offset, g.step_world, steps)
    gen = np.random.default_rng(steps + m)
    istate = torch.zeros(B, 4, dtype=torch.int32)
    want_z, want_k, want_n, want_more = [], [], [], []
    live = [b for b in range(B) if b % 5 != 3]                 # a sparse, ascending live list
    for b in range(B):
        kk = torch.nonzero(keep[b]).flatten().tolist()
        p = int(gen.integers(0, len(kk) + 1))
        lo = kk[p - 1] + 1 if p > 0 else 0                       # resume anywhere in (k_{p-1}, k_p]
        hi = kk[p] if p < len(kk) else 2 * steps
        k0 = int(gen.integers(lo, hi + 1))
        term = b % 11 == 0
        istate[b] = torch.tensor([k0, p, 0, 1 if term else 0], dtype=torch.int32)
        take = [] if term else kk[p:p + m]
        want_z.append(zc[b, take])
        want_n.append(len(take))
        more = (not term) and len(take) == m and p + m < steps and take[-1] + 1 < 2 * steps
        want_more.append(more)
        want_k.append(take[-1] + 1 if more else None)
    live_t = torch.tensor(live, dtype=torch.int32, device=DEV)
    ist = istate.to(DEV)
    A = len(live)
    live_out = sentinel_(torch.empty(A, dtype=torch.int32, device=DEV))
    g.march_resume(rays, 0.5, ist, live_t, A, m, live_out)                # grow the capacity buffers, then poison them
    for k in ("ert_rows", "ert_z"):
        sentinel_(g._cull[k])
    g._cull["ert_offsets"].fill_(SENT64)
    ist = istate.to(DEV)
    offs, rows, z, K, A_next = g.march_resume(rays, 0.5, ist, live_t, A, m, live_out)
    assert K == sum(want_n[b] for b in live)
    assert bits_equal(z.cpu(), torch.cat([want_z[b] for b in live]))
    assert bits_equal(rows.cpu(), torch.cat([rays.cpu()[b:b + 1].expand(want_n[b], 11) for b in live]))
    assert unwritten(z) == 0 and unwritten(rows) == 0
    cnt = (offs[1:A + 1] - offs[:A]).cpu()
    assert int(offs[0]) == 0 and cnt.tolist() == [want_n[b] for b in live]
    assert A_next == sum(want_more[b] for b in live)
    assert live_out[:A_next].cpu().tolist() == [b for b in live if want_more[b]]
    got = ist.cpu()
    for b in live:
        if want_n[b]:
            assert int(got[b, 1]) == int(istate[b, 1]) + want_n[b]
            if want_more[b]:
                assert int(got[b, 0]) == want_k[b]
    not_live = [b for b in range(B) if b % 5 == 3]
    assert torch.equal(got[not_live], istate[not_live])


# ------------------------------------------------------------------------------------------------ 3: the fold alone
def _hand_packed(lengths, seed):
    gen = torch.Generator().manual_seed(seed)
    offs = torch.zeros(len(lengths) + 1, dtype=torch.int64)
    offs[1:] = torch.cumsum(torch.tensor(lengths), 0)
    K = int(offs[-1])
    raw = torch.rand(K, 4, generator=gen)
    raw[:, 3] = torch.randn(K, generator=gen) * 2.0 + 2.0
    z = torch.sort(torch.rand(K, generator=gen) * 4 + 2).values
    return raw, z, offs


@pytest.mark.parametrize("eps", [0.0, 1e-4, 1e-2, 0.5])
def test_fold_matches_the_reference(eps):
    from nerf_meets_mlx_amd.rendering import render
    lengths = [0, 1, 5, 63, 64, 200, 1024, 7, 300, 40]
    raw, z, offs = _hand_packed(lengths, 3)
    raw[int(offs[3]) + 2, 3] = float("inf")                      # ray 3: opaque at its third sample
    raw[int(offs[8]), 3] = float("nan")                          # ray 8: NaN at its first sample (T = 1 >= eps)
    B = len(lengths)
    step = M.step_world(1024, 1.5)
    for white in (False, True):
        w_rgb, w_acc, w_depth, w_n = E.fold(raw, z, offs, step, eps, white)
        outs = []
        for split in (None, 3):                                   # one round, or every segment split into rounds of 3 samples
            ist = torch.zeros(B, 4, dtype=torch.int32, device=DEV)
            fst = torch.zeros(B, 6, dtype=torch.float32, device=DEV)
            live = torch.arange(B, dtype=torch.int32, device=DEV)
            render.ert_init(ist, fst, live, B)
            if split is None:
                render.ert_fold(raw.to(DEV), z.to(DEV), offs.to(DEV), live, B, ist, fst, step, eps)
            else:
                for r0 in range(0, max(lengths), split):
                    idx = [torch.arange(min(int(offs[b]) + r0, int(offs[b + 1])), min(int(offs[b]) + r0 + split, int(offs[b + 1])))
                           for b in range(B)]
                    o = torch.zeros(B + 1, dtype=torch.int64)
                    o[1:] = torch.cumsum(torch.tensor([len(i) for i in idx]), 0)
                    sel = torch.cat(idx)
                    render.ert_fold(raw[sel].contiguous().to(DEV), z[sel].to(DEV), o.to(DEV), live, B, ist, fst, step, eps)
            outs.append(render.ert_finish(ist, fst, white))
        for a, b in zip(outs[0], outs[1]):
            assert bits_equal(a.view(torch.int32), b.view(torch.int32))
        rgb, acc, depth, n = (t.cpu() for t in outs[0])
        ok = [b for b in range(B) if b != 8]
        assert bool(torch.isnan(rgb[8]).all()) and bool(torch.isfinite(rgb[ok]).all()) and bool(torch.isfinite(acc[ok]).all())
        assert float(acc[0]) == 0.0 and float(depth[0]) == 0.0 and rgb[0].tolist() == ([1.0] * 3 if white else [0.0] * 3)
        if eps > 0:
            assert int(n[3]) == 3                                  # +inf terminates right after itself
        # the stop index: the reference's, except where its T lies within 1e-5 relative of eps
        T_got = E.transmittance_at_stop(raw, offs, step, n)
        T_ref = E.transmittance_at_stop(raw, offs, step, w_n)
        for b in ok:
            if int(n[b]) != int(w_n[b]):
                assert eps > 0 and min(abs(float(T_got[b]) / eps - 1), abs(float(T_ref[b]) / eps - 1)) < 1e-5, b
                continue
            assert float((rgb[b] - w_rgb[b]).abs().max()) <= 2e-6 and abs(float(acc[b] - w_acc[b])) <= 2e-6
            assert abs(float(depth[b] - w_depth[b])) <= 1e-5 * max(1.0, abs(float(w_depth[b])))


# ------------------------------------------------------------------------------------------------ 4: the error bound
@pytest.mark.parametrize("eps", [1e-4, 1e-2, 0.5])
def test_error_bound_against_the_one_shot_renderer(eps):
    f = _field()
    g = _grid(f, 1024)
    _random_bits(g, 0.6, 9)
    dense = _Dense(f, 3.0)
    rays = _rays(2048, 7)
    w_rgb, w_acc, w_depth, w_n = _one_shot(g, dense, rays, 0.5, True, True)
    offs, rows, z, K = g.march(rays, 0.5)
    c_bg = float((dense.query_packed(rows, z)[:, 0, :3] - 1.0).abs().max())     # max |c - bg| (colours are not squashed)
    o = g.render_ert(dense, rays, 0.5, eps, True)
    n = o["samples"].long()
    assert bool((n <= w_n).all())
    d_rgb = (o["rgb"] - w_rgb).abs().max(1).values
    d_acc = w_acc - o["acc"]
    tol = 4e-6                                                   # the packed and the serial sums round differently
    assert float(d_rgb.max()) < eps * max(1.0, c_bg) + tol
    assert bool((d_acc >= -tol).all()) and float(d_acc.max()) < eps + tol
    has = w_n > 0
    early = int(((n < w_n) & has).sum())
    print(f"\neps {eps}: {early} of {int(has.sum())} rays with samples stop early; samples {int(n.sum())} of {int(w_n.sum())}")
    if eps == 1e-2:
        assert early >= int(has.sum()) // 4


# ------------------------------------------------------------------------------------------------ 5: schedule independence
def test_outputs_do_not_depend_on_the_schedule():
    f = _field()
    g = _grid(f, 256)
    _random_bits(g, 0.6, 10)
    dense = _Dense(f, 2.0)
    rays = _rays(3000, 8)
    jit = torch.rand(3000, generator=torch.Generator().manual_seed(13)).float().to(DEV)
    keys = ("rgb", "acc", "depth", "samples")

    def run(r, j, **kw):
        o = g.render_ert(dense, r, j, 1e-2, True, **kw)
        return [o[k].clone() for k in keys]

    ref = run(rays, jit)
    assert g.last_ert["rounds"] > 1
    chunks = [run(rays[s:s + 1000], jit[s:s + 1000]) for s in range(0, 3000, 1000)]
    rev = [t.flip(0) for t in run(rays.flip(0).contiguous(), jit.flip(0).contiguous())]
    variants = [[torch.cat([c[i] for c in chunks]) for i in range(4)], rev, run(rays, jit, slots=1), run(rays, jit, slots=64)]
    for v in variants:
        for a, b in zip(v, ref):
            assert bits_equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------ 6: poisoned buffers
def test_every_output_is_written_over_poisoned_buffers():
    from nerf_meets_mlx_amd import _native as N
    f = _field()
    g = _grid(f, 1024)
    _random_bits(g, 0.5, 11)
    dense = _Dense(f, 2.0)
    rays = _rays(1024, 9)
    a = g.render_ert(dense, rays, 0.5, 1e-3, True)
    a = {k: v.clone() for k, v in a.items()}
    for k, t in g._cull.items():
        if k.startswith("ert_"):
            if t.dtype == torch.uint8:
                t.fill_(0xA5)
            else:
                t.view(torch.int32).fill_(0x7FE5A5A5)
    b = g.render_ert(dense, rays, 0.5, 1e-3, True)
    for k in a:
        assert bits_equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    # the finish writes every output
    ist, fst = g._cull["ert_istate"][:4 * 1024].view(1024, 4), g._cull["ert_fstate"][:6 * 1024].view(1024, 6)
    outs = [sentinel_(torch.empty(*s, dtype=torch.float32, device=DEV)) for s in ((1024, 3), (1024,), (1024,), (1024,))]
    N.check(N.lib().nerf_ert_finish(N.ptr(ist), N.ptr(fst), 1024, 1, *(N.ptr(t) for t in outs), N.stream()))
    assert all(unwritten(t) == 0 for t in outs)
    assert bits_equal(outs[0], a["rgb"]) and bits_equal(outs[3], a["samples"].view(torch.float32))


# ------------------------------------------------------------------------------------------------ 7: trainer
def _trainer(hw, views, arm, eps=None, steps=256):
    from nerf_meets_mlx_amd.dataset import synthetic
    from nerf_meets_mlx_amd.engine.ngp import NGPTrainer
    imgs, poses, rposes, hwf, K = synthetic.make_dataset(hw, hw, views + 1, seed=0, device=DEV)
    kw = dict(occupancy_grid=arm != "free", march_steps=steps if arm == "march" else None, min_transmittance=eps)
    tr = NGPTrainer(imgs[:-1], poses[:-1], K, N_rand=256, n_depth_samples=64, seed=4, device=DEV, log2_hashmap_size=14, **kw)
    return tr, imgs[-1], poses[-1]


def test_trainer_training_is_untouched_and_the_frame_is_within_eps():
    from nerf_meets_mlx_amd.engine.occupancy import WARMUP
    eps = 1e-4
    a, gt, pose = _trainer(48, 8, "march", eps)
    b, _, _ = _trainer(48, 8, "march")
    for _ in range(WARMUP + 200):
        la, lb = a.train_step()["loss_coarse"], b.train_step()["loss_coarse"]
        # the reported loss is a sum of float atomics (nerf_composite_packed_mse_backward): its last bits vary from run to run
        # with or without eps; the gradients, and so every parameter below, do not
        assert abs(float(la) - float(lb)) <= 1e-6 * abs(float(lb))
    for x, y in ((a.field.mlp.params, b.field.mlp.params), (a.field.enc.tables, b.field.enc.tables),
                 (a.grid.density, b.grid.density), (a.grid.bits, b.grid.bits)):
        assert bits_equal(x, y)
    c2w = pose[:3, :4].numpy()
    img_eps = a.render_frame(c2w, shard=False)
    a.min_transmittance = None
    img_full = a.render_frame(c2w, shard=False)
    a.min_transmittance = eps
    d = float((img_eps - img_full).abs().max())
    assert d <= eps + 1e-6, d
    # samples per ray on the frame's rays: the round renderer's against the one-shot march's
    from nerf_meets_mlx_amd.rendering import ray
    rays = ray.gen_rays(a.H, a.W, a.K, c2w, a.near, a.far, torch.arange(a.H * a.W, device=DEV))
    s_eps = float(a.render_rays(rays, aux=True)["samples"].double().mean())
    a.min_transmittance = None
    s_full = float(a.render_rays(rays, aux=True)["samples"].double().mean())
    a.min_transmittance = eps
    print(f"\nert trainer hw48: samples/ray {s_eps:.2f} (one-shot {s_full:.2f}); max |d| {d:.2e}; PSNR {a.psnr(c2w, gt):.2f}")
    assert s_eps <= s_full


@pytest.mark.parametrize("arm", ["free", "cull", "march", "ert"])
def test_render_rays_aux_in_every_mode(arm):
    from nerf_meets_mlx_amd.rendering import ray
    tr, _, pose = _trainer(16, 3, "march" if arm == "ert" else arm, 1e-3 if arm == "ert" else None)
    for _ in range(20):
        tr.train_step()
    rays = ray.gen_rays(16, 16, tr.K, pose[:3, :4].numpy(), tr.near, tr.far, torch.arange(256, device=DEV))
    rgb = tr.render_rays(rays)
    o = tr.render_rays(rays, aux=True)
    assert torch.is_tensor(rgb) and rgb.shape == (256, 3)
    assert set(o) == ({"rgb", "acc", "depth", "samples"} if arm in ("march", "ert") else {"rgb", "acc", "depth"})
    assert bits_equal(o["rgb"], rgb)
    acc, depth = o["acc"], o["depth"]
    assert acc.shape == (256,) and depth.shape == (256,) and bool(torch.isfinite(acc).all()) and bool(torch.isfinite(depth).all())
    if arm in ("free", "cull"):                                   # the 64-sample composite of the same samples
        from nerf_meets_mlx_amd import sampling
        from nerf_meets_mlx_amd.rendering import render
        z = sampling.sample_coarse(rays, tr.n)
        raw = tr.field.query(rays, z, grid=tr._grid_for_step())
        _, _, w_acc, _, w_depth = render.composite(raw, z, rays, 0.0, tr.white_bkgd)
        assert bits_equal(acc, w_acc) and bits_equal(depth, w_depth)
        return
    assert o["samples"].dtype == torch.int32 and int(o["samples"].sum()) > 0
    tr.min_transmittance = None
    full = tr.render_rays(rays, aux=True)
    if arm == "march":                                            # the one-shot march and packed compositing
        w_rgb, w_acc, w_depth, w_n = _one_shot(tr.grid, tr.field, rays.contiguous(), 0.5, False, tr.white_bkgd)
        assert bits_equal(acc, w_acc) and bits_equal(depth, w_depth) and torch.equal(o["samples"].long(), w_n)
        assert bits_equal(full["rgb"], rgb)
    else:
        assert bool((o["samples"] <= full["samples"]).all())
        assert float((full["acc"] - o["acc"]).max()) < 1e-3 + 4e-6
