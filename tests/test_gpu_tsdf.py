"""TSDF fusion on the GPU (csrc/tsdf.hip, engine/mesh/tsdf.py TSDFVolume, NGPTrainer.render_depth / extract_mesh_tsdf) against the
float32 emulation of tests/_tsdf_ref.py: D, Wt and flags bit for bit (compared as integers) on maps that reach every branch of
the per-voxel rule, batched against single-view calls, the finish rule into a poisoned output, the empty volume, the 6-view
sphere through marching cubes, and a march-mode trainer's fused mesh."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import _mesh_ref as M
from tests import _tsdf_ref as T
from tests._poison import bits_equal, sentinel_, unwritten

pytestmark = pytest.mark.gpu
DEV = "cuda"
_F = np.float32
LO, HI = [-1.0] * 3, [1.0] * 3


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"


# ------------------------------------------------------------------------------------------------ fixtures
def _spoil(depth, acc, rng):
    """Sphere maps with a fifth of the pixels replaced: semi-transparent pixels on both sides of acc_min = 0.5 (depth = acc z,
    as a compositor gives), NaN in acc, NaN in depth, acc = depth = 0 (already there wherever the sphere is missed), and
    acc = depth = inf (a NaN distance)."""
    depth, acc = depth.copy(), acc.copy()
    n = depth.size
    idx = rng.permutation(n)
    k = n // 20
    a = rng.uniform(0.05, 1.0, k).astype(_F)
    acc[idx[:k]] = a
    depth[idx[:k]] = (a * rng.uniform(1.5, 4.5, k).astype(_F)).astype(_F)
    acc[idx[k:2 * k]] = np.nan
    depth[idx[2 * k:3 * k]] = np.nan
    acc[idx[3 * k:4 * k]] = 0.0
    depth[idx[3 * k:4 * k]] = 0.0
    acc[idx[4 * k:4 * k + k // 4]] = np.inf                  # inf / inf: a NaN distance
    depth[idx[4 * k:4 * k + k // 4]] = np.inf
    return depth, acc


@functools.lru_cache(maxsize=None)
def _views(n, H, W, seed=7, inside=True):
    """(views [n, 16], depth [n, H W], acc [n, H W]): cameras around a sphere of radius 0.55 centred at (0.1, -0.05, 0.05), the
    second one INSIDE the lattice's box (voxels behind it have zc <= 0).  Computed once per module run, never changed."""
    rng = np.random.default_rng(seed)
    K = T.intrinsics(H, W, fov=0.8)
    views, depth, acc = [], [], []
    for s in range(n):
        if inside and s == 1:
            eye = np.array([0.75, -0.6, 0.3])
        else:
            d = rng.standard_normal(3)
            eye = 3.0 * d / np.linalg.norm(d)
        c2w = T.look_at(eye, target=(0.1, -0.05, 0.05))
        dm, am = _spoil(*T.sphere_maps(c2w, K, H, W, 0.55, centre=(0.1, -0.05, 0.05)), rng)
        views.append(T.view_floats(c2w, K))
        depth.append(dm)
        acc.append(am)
    out = np.stack(views), np.stack(depth), np.stack(acc)
    for a in out:
        a.setflags(write=False)
    return out


class _State:
    """D, Wt, flags on the device, each with one spare sentinel element past the lattice."""

    def __init__(self, R, ref=None):
        self.R, n3 = R, R ** 3
        self.D = sentinel_(torch.empty(n3 + 1, dtype=torch.float32, device=DEV))
        self.Wt = sentinel_(torch.empty(n3 + 1, dtype=torch.float32, device=DEV))
        self.flags = torch.full((n3 + 1,), 0xA5, dtype=torch.uint8, device=DEV)
        if ref is None:
            from nerf_meets_mlx_amd import _native as N
            N.check(N.lib().nerf_tsdf_reset(N.ptr(self.D), N.ptr(self.Wt), N.ptr(self.flags), R, N.stream()))
        else:
            self.D[:n3] = torch.from_numpy(ref.D).to(DEV)
            self.Wt[:n3] = torch.from_numpy(ref.Wt).to(DEV)
            self.flags[:n3] = torch.from_numpy(ref.flags).to(DEV)

    def spare_intact(self):
        return unwritten(self.D[-1:]) == 1 and unwritten(self.Wt[-1:]) == 1 and int(self.flags[-1]) == 0xA5

    def bits(self):
        n3 = self.R ** 3
        return (self.D[:n3].view(torch.int32).cpu().numpy(), self.Wt[:n3].view(torch.int32).cpu().numpy(),
                self.flags[:n3].cpu().numpy())

    def equals(self, ref):
        d, w, f = self.bits()
        return (self.spare_intact() and np.array_equal(d, ref.D.view(np.int32)) and np.array_equal(w, ref.Wt.view(np.int32))
                and np.array_equal(f, ref.flags))


def _integrate(st, views, H, W, depth, acc, tau, acc_min, far, carve, lo=LO, hi=HI):
    from nerf_meets_mlx_amd import _native as N
    views = np.ascontiguousarray(views, _F).reshape(-1, 16)
    n = len(views)
    d = torch.from_numpy(np.array(depth, _F).reshape(n, H * W)).to(DEV)
    a = torch.from_numpy(np.array(acc, _F).reshape(n, H * W)).to(DEV)
    N.check(N.lib().nerf_tsdf_integrate(N.ptr(st.D), N.ptr(st.Wt), N.ptr(st.flags), st.R, (C.c_float * 3)(*lo), (C.c_float * 3)(*hi),
                                        views.ctypes.data_as(C.POINTER(C.c_float)) if n else None, n, H, W,
                                        N.ptr(d) if n else None, N.ptr(a) if n else None, tau, acc_min, far, int(carve), N.stream()))
    torch.cuda.synchronize()
    return st


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a.bits(), b.bits())) and a.spare_intact() and b.spare_intact()


# ------------------------------------------------------------------------------------------------ integrate, bit for bit
@pytest.mark.parametrize("carve", [True, False])
def test_integrate_matches_the_reference_bit_for_bit(carve):
    """R = 24 (R^3 is no multiple of the 256-lane workgroup), 40 x 56 maps, 3 views folded by 3 calls -- the third with far = 3,
    the middle of the box as seen from its camera at distance 3 -- and by one batched call with a common far."""
    R, H, W = 24, 40, 56
    views, depth, acc = _views(3, H, W)
    tau = T.default_trunc(R, LO, HI)
    fars = (6.0, 6.0, 3.0)
    ref, st = T.State(R), _State(R)
    for s in range(3):
        T.integrate(ref, LO, HI, views[s:s + 1], H, W, depth[s:s + 1], acc[s:s + 1], tau, 0.5, fars[s], carve)
        _integrate(st, views[s:s + 1], H, W, depth[s:s + 1], acc[s:s + 1], tau, 0.5, fars[s], carve)
        assert st.equals(ref), f"view {s}"
    # the fixture reaches every branch of the rule, counted on the reference's own classification of each view
    cls = [T.classify_view(R, LO, HI, views[s], H, W, depth[s], acc[s], tau, 0.5, fars[s], carve) for s in range(3)]
    count = lambda k: sum(int(c[k].sum()) for c in cls)
    assert int(cls[1]["behind"].sum()) > 100 and float(cls[1]["zc"].min()) < 0.0          # zc <= 0 behind the camera inside the box
    assert int(cls[0]["behind"].sum()) == 0
    for k in ("outside", "nan_acc", "nan_depth", "occluded", "nan_e", "surface"):
        assert count(k) > 50, k
    assert count("zero_pixel") > 1000                                                     # acc = 0 with depth = 0
    if carve:
        assert count("empty") > 1000 and int(cls[0]["low_skipped"].sum()) == 0
        assert int(cls[2]["low_skipped"].sum()) > 1000 and int(cls[2]["empty"].sum()) > 1000   # far = 3 cuts the carving mid-box
    else:
        assert count("empty") == 0 and count("low_skipped") > 1000
    semi = (acc[0] > 0.0) & (acc[0] < 1.0)
    assert int((semi & (acc[0] < 0.5)).sum()) > 20 and int((semi & (acc[0] >= 0.5)).sum()) > 20   # both sides of acc_min
    # and its outcomes: unseen, seen by some and by all views, occluded voxels, non-trivial means
    assert set(np.unique(ref.Wt).tolist()) == {0.0, 1.0, 2.0, 3.0} and 0 < int(ref.flags.sum()) < R ** 3
    assert len(np.unique(ref.D)) > 100 and float(ref.D.min()) < -0.5 and float(ref.D.max()) == 1.0
    batched_ref = T.integrate(T.State(R), LO, HI, views, H, W, depth, acc, tau, 0.5, 3.0, carve)
    assert _integrate(_State(R), views, H, W, depth, acc, tau, 0.5, 3.0, carve).equals(batched_ref)
    assert np.array_equal(batched_ref.Wt, ref.Wt) == (not carve)                          # far matters exactly when carving


def test_carving_and_far_change_the_result():
    R, H, W = 24, 40, 56
    views, depth, acc = _views(3, H, W)
    tau = T.default_trunc(R, LO, HI)
    on = T.integrate(T.State(R), LO, HI, views, H, W, depth, acc, tau, 0.5, 6.0, True)
    off = T.integrate(T.State(R), LO, HI, views, H, W, depth, acc, tau, 0.5, 6.0, False)
    assert (off.Wt <= on.Wt).all() and (off.Wt < on.Wt).any()
    got = _integrate(_State(R), views, H, W, depth, acc, tau, 0.5, 6.0, True)
    assert got.equals(on) and not got.equals(off)
    # another acc_min, another truncation, a box that is no cube
    lo, hi = [-1.0, -0.8, -1.2], [1.1, 0.9, 0.7]
    ref = T.integrate(T.State(R), lo, hi, views, H, W, depth, acc, 0.11, 0.9, 2.5, True)
    st = _State(R)
    _integrate(st, views, H, W, depth, acc, 0.11, 0.9, 2.5, True, lo=lo, hi=hi)
    assert st.equals(ref)


# ------------------------------------------------------------------------------------------------ batching
def test_one_batch_single_calls_and_a_split_are_bit_identical():
    R, H, W = 17, 24, 32
    views, depth, acc = _views(5, H, W, seed=11)
    tau = T.default_trunc(R, LO, HI)
    args = (tau, 0.5, 6.0, True)
    whole = _integrate(_State(R), views, H, W, depth, acc, *args)
    single = _State(R)
    for s in range(5):
        _integrate(single, views[s:s + 1], H, W, depth[s:s + 1], acc[s:s + 1], *args)
    split = _State(R)
    _integrate(split, views[:2], H, W, depth[:2], acc[:2], *args)
    _integrate(split, views[2:], H, W, depth[2:], acc[2:], *args)
    assert _same(whole, single) and _same(whole, split)
    assert whole.equals(T.integrate(T.State(R), LO, HI, views, H, W, depth, acc, *args))
    again = _integrate(_State(R), views, H, W, depth, acc, *args)                        # the same calls twice: the same bits
    assert _same(whole, again)
    # the order of the views is the order of the float32 recurrence: reversed, some means differ in the last place
    fwd = T.integrate(T.State(R), LO, HI, views, H, W, depth, acc, *args)
    rev = T.integrate(T.State(R), LO, HI, views[::-1], H, W, depth[::-1], acc[::-1], *args)
    got_rev = _integrate(_State(R), views[::-1], H, W, depth[::-1], acc[::-1], *args)
    assert got_rev.equals(rev)
    differ = int((fwd.D.view(np.int32) != rev.D.view(np.int32)).sum())
    print("voxels whose mean differs between the two orders:", differ, "of", R ** 3)
    assert differ > 0 and not _same(whole, got_rev)
    assert np.array_equal(fwd.Wt, rev.Wt) and np.array_equal(fwd.flags, rev.flags)       # counts and flags do not depend on it
    assert float(np.abs(fwd.D - rev.D).max()) < 1e-6


def test_seventeen_views_through_tsdfvolume_equal_seventeen_single_calls():
    from nerf_meets_mlx_amd.engine import mesh
    R, H, W = 17, 24, 32
    views, depth, acc = _views(17, H, W, seed=13)
    K = T.intrinsics(H, W, fov=0.8)
    c2w = views[:, :12].reshape(17, 3, 4)
    assert np.array_equal(mesh.tsdf_views(c2w, K), views)
    vol = mesh.TSDFVolume(R, LO, HI, device=DEV)
    assert vol.trunc == T.default_trunc(R, LO, HI)
    vol.integrate(torch.from_numpy(depth.copy()).to(DEV).reshape(17, H, W), torch.from_numpy(acc.copy()).to(DEV).reshape(17, H, W),
                  c2w, K, H, W, acc_min=0.5, far=6.0, carve=True)
    single = mesh.TSDFVolume(R, LO, HI, device=DEV)
    for s in range(17):
        single.integrate(torch.from_numpy(depth[s].copy()).to(DEV), torch.from_numpy(acc[s].copy()).to(DEV), c2w[s], K, H, W,
                         acc_min=0.5, far=6.0, carve=True)
    ref = T.integrate(T.State(R), LO, HI, views, H, W, depth, acc, vol.trunc, 0.5, 6.0, True)
    for v in (vol, single):
        assert np.array_equal(v.D.view(torch.int32).cpu().numpy(), ref.D.view(np.int32))
        assert np.array_equal(v.Wt.view(torch.int32).cpu().numpy(), ref.Wt.view(np.int32))
        assert np.array_equal(v.flags.cpu().numpy(), ref.flags)
    ref16 = T.integrate(T.State(R), LO, HI, views[:16], H, W, depth[:16], acc[:16], vol.trunc, 0.5, 6.0, True)
    assert not np.array_equal(ref16.Wt, ref.Wt) and float(ref.Wt.max()) >= 16.0                   # the second launch's view counts
    for bad in ({"acc_min": 0.0}, {"far": -1.0}, {"carve": 1}):
        with pytest.raises(ValueError):
            vol.integrate(torch.zeros(H * W, device=DEV), torch.zeros(H * W, device=DEV), c2w[0], K, H, W, **bad)
    with pytest.raises(ValueError):
        vol.integrate(torch.zeros(H * W + 1, device=DEV), torch.zeros(H * W, device=DEV), c2w[0], K, H, W)
    with pytest.raises(ValueError):
        vol.integrate(torch.zeros(H * W, device=DEV), torch.zeros(2, H * W, device=DEV), c2w[0], K, H, W)
    assert np.array_equal(vol.D.view(torch.int32).cpu().numpy(), ref.D.view(np.int32))           # refused calls changed nothing


# ------------------------------------------------------------------------------------------------ finish, reset, empty
@pytest.mark.parametrize("R", [2, 24])
@pytest.mark.parametrize("min_views", [1, 2])
def test_volume_writes_every_voxel_by_the_three_branch_rule(R, min_views):
    from nerf_meets_mlx_amd import _native as N
    rng = np.random.default_rng(R)
    ref = T.State(R)
    n3 = R ** 3
    ref.D[:] = rng.uniform(-1.0, 1.0, n3).astype(_F)
    ref.Wt[:] = rng.integers(0, 4, n3).astype(_F)
    ref.flags[:] = rng.integers(0, 2, n3).astype(np.uint8)
    ref.Wt[:8] = np.array([0, 0, 1, 1, 2, 2, 3, 0], _F)                                          # R = 2: every branch by hand
    ref.flags[:8] = np.array([0, 1, 0, 1, 0, 1, 0, 1], np.uint8)
    want = T.volume(ref, min_views)
    assert {-1.0, 1.0} <= set(np.unique(want).tolist()) and len(np.unique(want)) > 2              # all three branches
    st = _State(R, ref)
    out = sentinel_(torch.empty(n3 + 1, dtype=torch.float32, device=DEV))
    N.check(N.lib().nerf_tsdf_volume(N.ptr(st.D), N.ptr(st.Wt), N.ptr(st.flags), R, min_views, N.ptr(out), N.stream()))
    assert unwritten(out) == 1 and unwritten(out[-1:]) == 1
    assert bits_equal(out[:n3].cpu(), torch.from_numpy(want.reshape(-1)))
    assert st.equals(ref)                                                                         # the state is read only
    N.check(N.lib().nerf_tsdf_reset(N.ptr(st.D), N.ptr(st.Wt), N.ptr(st.flags), R, N.stream()))
    assert st.equals(T.State(R))


def test_tsdfvolume_reset_and_the_empty_volume():
    from nerf_meets_mlx_amd.engine import mesh
    R, H, W = 9, 24, 32
    views, depth, acc = _views(2, H, W, seed=11)
    K = T.intrinsics(H, W, fov=0.8)
    t = mesh.TSDFVolume(R, LO, HI, device=DEV)
    empty = t.volume()
    assert empty.shape == (R, R, R) and empty.dtype == torch.float32 and bool((empty == -1.0).all())
    m = mesh.marching_cubes(empty, 0.0, LO, HI)
    assert m.verts.shape == (0, 3) and m.faces.shape == (0, 3)
    t.integrate(torch.from_numpy(depth.copy()).to(DEV), torch.from_numpy(acc.copy()).to(DEV), views[:, :12].reshape(2, 3, 4), K, H, W)
    assert float(t.Wt.max()) == 2.0 and not bool((t.volume() == -1.0).all())
    before = (t.D.clone(), t.Wt.clone(), t.flags.clone())
    # no views: through the class (an empty stack) and through the C entry (n = 0, NULL views and maps)
    t.integrate(torch.zeros(0, H * W, device=DEV), torch.zeros(0, H * W, device=DEV), np.zeros((0, 3, 4)), K, H, W)
    st = _State(R)
    st.D[:-1], st.Wt[:-1], st.flags[:-1] = t.D, t.Wt, t.flags
    _integrate(st, np.zeros((0, 16), _F), H, W, np.zeros((0, H * W), _F), np.zeros((0, H * W), _F), t.trunc, 0.5, 6.0, True)
    assert st.spare_intact()
    for a, b, c in zip(before, (t.D, t.Wt, t.flags), (st.D[:-1], st.Wt[:-1], st.flags[:-1])):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)) and torch.equal(a.view(torch.uint8), c.view(torch.uint8))
    t.reset()
    assert not t.D.any() and not t.Wt.any() and not t.flags.any() and bool((t.volume(3) == -1.0).all())
    for mv in (0, 1.5, True):
        with pytest.raises(ValueError):
            t.volume(mv)


# ------------------------------------------------------------------------------------------------ mesh
def test_six_view_sphere_mesh_is_closed_and_equals_the_reference():
    from nerf_meets_mlx_amd.engine import mesh
    ref, lo, hi, tau, views, depth, acc, H, W = T.sphere_fixture()
    R = ref.R
    assert R == 32
    t = mesh.TSDFVolume(R, lo, hi, device=DEV)
    t.integrate(torch.from_numpy(depth).to(DEV), torch.from_numpy(acc).to(DEV), views[:, :12].reshape(6, 3, 4),
                T.intrinsics(H, W, fov=0.9), H, W, acc_min=0.5, far=6.0, carve=True)
    vol = t.volume()
    want_vol = T.volume(ref, 1)
    assert bits_equal(vol.cpu(), torch.from_numpy(want_vol))
    got = mesh.marching_cubes(vol, 0.0, lo, hi)
    v, f, n = M.marching_cubes(want_vol, 0.0, lo, hi)
    assert len(v) > 1000 and set(M.undirected_edge_counts(f).tolist()) == {2}                     # each edge in exactly two faces
    assert bits_equal(got.verts.cpu(), torch.from_numpy(v)) and torch.equal(got.faces.cpu(), torch.from_numpy(f))
    assert set(M.undirected_edge_counts(got.faces.cpu().numpy()).tolist()) == {2}


# ------------------------------------------------------------------------------------------------ the depth convention
def test_every_renderers_depth_over_acc_is_distance_along_the_optical_axis():
    """The fusion reads depth / acc as the axial distance of the surface.  A wall perpendicular to the optical axis at axial
    distance A = 3, given to the three compositors behind render_rays(aux=True) -- the 64-sample one, the march's packed one and
    the early-termination fold -- as densities on the sample positions o + z d of nerf_ray_gen's rays (90 degree field of view:
    |d| up to 1.7).  The first sample behind the wall takes all the weight, so depth / acc lies in [A, A + dz] on every ray,
    where the Euclidean distance A |d| is up to 2.1 farther."""
    from nerf_meets_mlx_amd.rendering import ray, render
    H = W = 16
    K = np.array([[8.0, 0.0, 8.0], [0.0, 8.0, 8.0], [0.0, 0.0, 1.0]])
    c2w = T.look_at((2.0, -1.5, 1.0))
    rays = ray.gen_rays(H, W, K, c2w, 2.0, 4.0, torch.arange(H * W, device=DEV))
    o, d = rays[:, :3].double().cpu(), rays[:, 3:6].double().cpu()
    fwd = -torch.from_numpy(c2w[:3, 2])                                                    # the optical axis in the world
    assert float(((d @ fwd) - 1.0).abs().max()) < 1e-6                                    # camera z of every d is -1
    norm = d.norm(dim=1)
    assert float(norm.max()) > 1.6
    A, n = 3.0, 64
    z = torch.linspace(2.0, 4.0, n, dtype=torch.float32).repeat(H * W, 1)
    dz = 2.0 / (n - 1)
    pts = o[:, None, :] + z.double()[..., None] * d[:, None, :]
    behind = ((pts - o[:, None, :]) @ fwd) >= A                                           # geometry, not z: beyond the wall
    assert bool(behind.any(1).all()) and not bool(behind[:, 0].any())
    zd = z.to(DEV)

    def check(depth, acc, what):
        got = (depth / acc).double().cpu()
        print(what, "depth / acc in", float(got.min()), float(got.max()), "euclidean up to", float((A * norm).max()))
        assert float(acc.min()) > 0.999, what
        assert float(got.min()) >= A - 1e-5 and float(got.max()) <= A + dz + 1e-5, what
        assert float((A * norm - got).max()) > 1.5, what

    raw = torch.zeros(H * W, n, 4)
    raw[..., 3] = torch.where(behind, 1e4, 0.0)                                           # relu density
    _, _, acc, _, depth = render.composite(raw.to(DEV), zd, rays, 0.0, False)
    check(depth, acc, "64-sample compositor")
    praw = torch.zeros(H * W * n, 4)
    praw[:, 3] = torch.where(behind.reshape(-1), 10.0, -30.0)                             # exp density
    praw, pz = praw.to(DEV), zd.reshape(-1).contiguous()
    offsets = torch.arange(0, H * W * n + 1, n, dtype=torch.int64, device=DEV)
    _, acc, depth, _ = render.composite_packed_render(praw, pz, offsets, rays, 0.05, False)
    check(depth, acc, "packed compositor")
    B = H * W
    istate = torch.empty(B, 4, dtype=torch.int32, device=DEV)
    fstate = torch.empty(B, 6, dtype=torch.float32, device=DEV)
    live = torch.empty(B, dtype=torch.int32, device=DEV)
    render.ert_init(istate, fstate, live, B)
    render.ert_fold(praw, pz, offsets, live, B, istate, fstate, 0.05, 1e-4)
    _, acc, depth, _ = render.ert_finish(istate, fstate, False)
    check(depth, acc, "early-termination fold")


# ------------------------------------------------------------------------------------------------ trainer
def test_march_trainer_extract_mesh_tsdf():
    """hw 48, march mode, 50 iterations, R = 32: shapes, dtypes, colours, reproducibility, the composition with the component
    filter and the opening, and the argument checks.  Nothing about quality at this training length."""
    from nerf_meets_mlx_amd.dataset import synthetic
    from nerf_meets_mlx_amd.engine import mesh
    from nerf_meets_mlx_amd.engine.ngp import NGPTrainer
    imgs, poses, _, _, K = synthetic.make_dataset(48, 48, 8, seed=0, device=DEV)
    tr = NGPTrainer(imgs, poses, K, N_rand=1024, n_depth_samples=64, seed=4, device=DEV, log2_hashmap_size=14,
                    occupancy_grid=True, march_steps=1024)
    for _ in range(50):
        tr.train_step()
    R, lo, hi = 32, [-1.5] * 3, [1.5] * 3
    depth, acc = tr.render_depth(poses[0])
    assert depth.shape == acc.shape == (48, 48) and depth.dtype == acc.dtype == torch.float32
    assert bool(torch.isfinite(depth).all()) and 0.0 <= float(acc.min()) and float(acc.max()) <= 1.0 + 1e-5
    print("acc mean", float(acc.mean()), "max", float(acc.max()), "pixels >= 0.5:", int((acc >= 0.5).sum()))
    a = tr.extract_mesh_tsdf(resolution=R)
    V, F = a.verts.shape[0], a.faces.shape[0]
    print("V, F", V, F)
    assert V > 0 and F > 0
    assert a.verts.shape == (V, 3) and a.normals.shape == (V, 3) and a.colors.shape == (V, 3) and a.faces.shape == (F, 3)
    assert a.verts.dtype == a.normals.dtype == a.colors.dtype == torch.float32 and a.faces.dtype == torch.int32
    assert 0.0 <= float(a.colors.min()) and float(a.colors.max()) <= 1.0
    assert 0 <= int(a.faces.min()) and int(a.faces.max()) < V
    assert float(a.verts.min()) >= -1.5 and float(a.verts.max()) <= 1.5
    b = tr.extract_mesh_tsdf(resolution=R)
    assert bits_equal(a.verts, b.verts) and torch.equal(a.faces, b.faces) and bits_equal(a.colors, b.colors)
    # by hand: render, fuse, finish, marching cubes, colours
    t = mesh.TSDFVolume(R, lo, hi, device=DEV)
    maps = [tr.render_depth(p) for p in poses]
    t.integrate(torch.stack([m[0] for m in maps]), torch.stack([m[1] for m in maps]), poses, K, 48, 48, acc_min=0.5, far=tr.far)
    want, rows = mesh._marching_cubes(t.volume(1), 0.0, lo, hi, True)
    assert bits_equal(a.verts, want.verts) and torch.equal(a.faces, want.faces)
    assert bits_equal(a.colors, mesh.vertex_colors(tr._mesh_field()[0], rows))
    two = tr.extract_mesh_tsdf(resolution=R, poses=poses[:2], colors=False)
    assert two.colors is None and (two.verts.shape != a.verts.shape or not bits_equal(two.verts, a.verts))
    big = tr.extract_mesh_tsdf(resolution=R, largest_only=True, colors=False)
    assert 0 < big.verts.shape[0] <= V
    assert bits_equal(big.verts, mesh.marching_cubes(mesh.filter_components(t.volume(1), 0.0, 0, True), 0.0, lo, hi).verts)
    opened = tr.extract_mesh_tsdf(resolution=R, largest_only=True, opening_radius=1, colors=False)
    assert bits_equal(opened.verts, mesh.marching_cubes(mesh.open_components(t.volume(1), 0.0, 1, 0, True), 0.0, lo, hi).verts)
    strict = tr.extract_mesh_tsdf(resolution=R, min_views=8, carve=False, colors=False)
    assert strict.faces.dtype == torch.int32
    # every argument error fires before any launch: the fusion state is not even allocated
    torch.cuda.synchronize()
    mem = torch.cuda.memory_allocated()
    for bad in ({"resolution": 1}, {"resolution": 513}, {"trunc": 0.0}, {"trunc": float("nan")}, {"acc_min": 0.0}, {"acc_min": 1.5},
                {"carve": 1}, {"min_views": 0}, {"min_views": 1.5}, {"min_component": -1}, {"largest_only": 1},
                {"opening_radius": 17}, {"aabb": ([0.0] * 3, [0.0] * 3)}, {"poses": np.zeros((2, 2, 4))},
                {"poses": np.full((1, 3, 4), np.nan)}):
        with pytest.raises(ValueError):
            tr.extract_mesh_tsdf(**{"resolution": R, **bad})
    assert torch.cuda.memory_allocated() == mem
