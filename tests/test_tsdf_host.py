"""TSDF fusion, host side (no GPU): the argument checks of engine/mesh/tsdf.py, and on the reference tests/_tsdf_ref.py the
properties include/nerf_hip.h "TSDF fusion" relies on -- the fused sphere's zero crossing sits at the true radius, the depth
convention (depth / acc is distance along the optical axis) against the synthetic teacher, the three branches of the finish
rule, and that the +1 behind a surface leaves no inner shell; the exported symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import _mesh_ref as M
from tests import _tsdf_ref as T

_F = np.float32


# ------------------------------------------------------------------------------------------------ argument checks
def test_check_tsdf_args_accepts_and_normalises():
    from nerf_meets_mlx_amd.engine import mesh
    assert mesh.check_tsdf_args() == (None, 0.5, 1.0, True, 1, 1, 1)
    assert mesh.check_tsdf_args(0.25, 1, 6, False, 3, 40, 56) == (0.25, 1.0, 6.0, False, 3, 40, 56)
    assert mesh.check_tsdf_args(np.float32(0.5), np.float64(1e-3), 2.5, True, np.int64(2), np.int32(8), 1 << 24)[4:] == (2, 8, 1 << 24)


@pytest.mark.parametrize("kw", [
    {"trunc": 0.0}, {"trunc": -1.0}, {"trunc": float("nan")}, {"trunc": float("inf")}, {"trunc": True}, {"trunc": "0.1"},
    {"acc_min": 0.0}, {"acc_min": -0.5}, {"acc_min": 1.5}, {"acc_min": float("nan")}, {"acc_min": None}, {"acc_min": True},
    {"far": 0.0}, {"far": -2.0}, {"far": float("inf")}, {"far": float("nan")}, {"far": None},
    {"carve": 1}, {"carve": 0}, {"carve": None},
    {"min_views": 0}, {"min_views": -1}, {"min_views": 1.0}, {"min_views": True}, {"min_views": None},
    {"H": 0}, {"H": -4}, {"H": 2.0}, {"H": (1 << 24) + 1}, {"H": True}, {"W": 0}, {"W": -1}, {"W": None}, {"W": (1 << 24) + 1},
])
def test_check_tsdf_args_refuses(kw):
    from nerf_meets_mlx_amd.engine import mesh
    with pytest.raises(ValueError):
        mesh.check_tsdf_args(**kw)


def test_views_and_volume_refuse_bad_arguments_without_a_device():
    from nerf_meets_mlx_amd.engine import mesh
    K = T.intrinsics(8, 8)
    good = T.look_at((3.0, 0.0, 0.0))
    v = mesh.tsdf_views(good, K)
    assert v.dtype == np.float32 and v.shape == (1, 16) and np.array_equal(v[0], T.view_floats(good, K))
    four = np.concatenate([good, [[0.0, 0.0, 0.0, 1.0]]])
    assert np.array_equal(mesh.tsdf_views(torch.from_numpy(np.stack([four, four])), K), np.concatenate([v, v]))
    bad_pose = good.copy()
    bad_pose[1, 2] = np.nan
    for c2w, k in ((np.zeros((3, 3)), K), (np.zeros((2, 5, 4)), K), (np.zeros(12), K), (good, np.zeros((4, 4))), (bad_pose, K),
                   (good, np.where(K > 0, np.inf, K))):
        with pytest.raises(ValueError):
            mesh.tsdf_views(c2w, k)
    # the constructor checks its arguments before it allocates on a device
    for args in ((1, [-1.0] * 3, [1.0] * 3), (513, [-1.0] * 3, [1.0] * 3), (8, [1.0] * 3, [1.0] * 3), (8, [-1.0] * 2, [1.0] * 3),
                 (8, [-1.0] * 3, [1.0, 1.0, float("inf")])):
        with pytest.raises(ValueError):
            mesh.TSDFVolume(*args, device="cpu")
    for trunc in (0.0, -0.1, float("nan"), 1e-60):
        with pytest.raises(ValueError):
            mesh.TSDFVolume(8, [-1.0] * 3, [1.0] * 3, trunc=trunc, device="cpu")


def test_library_exports_and_header_declares_the_entries():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "nerf_hip.h")) as fh:
        header = fh.read()
    assert "TSDF fusion (no reference counterpart)" in header and re.search(r"#define NERF_TSDF_MAX_VIEWS 16\b", header)
    assert re.search(r"#define NERF_ABI_VERSION 3\b", header)
    from nerf_meets_mlx_amd import _native as N
    from nerf_meets_mlx_amd.engine import mesh
    assert mesh.TSDF_MAX_VIEWS == T.MAX_VIEWS == 16
    L = N.lib()
    for name in ("nerf_tsdf_reset", "nerf_tsdf_integrate", "nerf_tsdf_volume"):
        assert re.search(r"\bint %s\(" % name, header) and name in N.SIGNATURES
        assert getattr(L, name).restype is C.c_int
    assert L.nerf_abi_version() == 3


def test_c_entry_points_refuse_bad_arguments_before_any_launch():
    from nerf_meets_mlx_amd import _native as N
    L = N.lib()
    fake = C.c_void_p(0x1000)                                          # never dereferenced: every call below fails its checks first
    E_NULL, E_SHAPE = -1, -2
    f3 = lambda *x: (C.c_float * 3)(*x)
    view = (C.c_float * 32)(*([float(x) for x in T.view_floats(T.look_at((3.0, 0.0, 0.0)), T.intrinsics(8, 8))] * 2))

    def integrate(R=8, lo=(-1.0,) * 3, hi=(1.0,) * 3, views=view, n=1, H=8, W=8, tau=0.25, acc_min=0.5, far=6.0, carve=1,
                  state=(fake,) * 3, maps=(fake,) * 2):
        return L.nerf_tsdf_integrate(state[0], state[1], state[2], R, None if lo is None else f3(*lo), None if hi is None else f3(*hi),
                                     views, n, H, W, maps[0], maps[1], tau, acc_min, far, carve, None)

    assert integrate(maps=(None, fake)) == E_NULL and integrate(maps=(fake, None)) == E_NULL      # valid values reach the pointers
    assert integrate(views=None) == E_NULL and integrate(lo=None) == E_NULL and integrate(hi=None) == E_NULL
    for k in range(3):
        assert integrate(state=tuple(None if q == k else fake for q in range(3))) == E_NULL
        assert integrate(n=0, state=tuple(None if q == k else fake for q in range(3))) == E_NULL
    assert integrate(n=0, views=None, maps=(None, None)) == 0                                     # n = 0: nothing to launch
    for R in (1, 513, 0, -3):
        assert integrate(R=R) == E_SHAPE
        assert L.nerf_tsdf_reset(fake, fake, fake, R, None) == E_SHAPE
        assert L.nerf_tsdf_volume(fake, fake, fake, R, 1, fake, None) == E_SHAPE
    assert integrate(lo=(1.0, -1.0, -1.0)) == E_SHAPE and integrate(hi=(1.0, float("nan"), 1.0)) == E_SHAPE
    assert integrate(lo=(float("-inf"), -1.0, -1.0)) == E_SHAPE
    for n in (-1, 17, 1000):
        assert integrate(n=n) == E_SHAPE
    for bad in (0, -1):
        assert integrate(H=bad) == E_SHAPE and integrate(W=bad) == E_SHAPE
    assert integrate(H=(1 << 24) + 1) == E_SHAPE
    for bad in (0.0, -0.25, float("nan"), float("inf")):
        assert integrate(tau=bad) == E_SHAPE and integrate(far=bad) == E_SHAPE
    for bad in (0.0, -0.5, 1.0001, float("nan")):
        assert integrate(acc_min=bad) == E_SHAPE
    assert integrate(acc_min=1.0, maps=(None, None)) == E_NULL                                    # 1 is allowed
    for bad in (2, -1):
        assert integrate(carve=bad) == E_SHAPE
    for q in range(16):                                                                           # every camera number, second view
        for x in (float("nan"), float("inf")):
            v = (C.c_float * 32)(*view)
            v[16 + q] = x
            assert integrate(views=v, n=2) == E_SHAPE
            assert integrate(views=v, n=1, maps=(None, None)) == E_NULL                           # beyond n: not looked at
    for mv in (0, -1):
        assert L.nerf_tsdf_volume(fake, fake, fake, 8, mv, fake, None) == E_SHAPE
    for k in range(4):
        p = [None if q == k else fake for q in range(4)]
        assert L.nerf_tsdf_volume(p[0], p[1], p[2], 8, 1, p[3], None) == E_NULL
    for k in range(3):
        p = [None if q == k else fake for q in range(3)]
        assert L.nerf_tsdf_reset(p[0], p[1], p[2], 8, None) == E_NULL


# ------------------------------------------------------------------------------------------------ the reference's properties
def test_six_view_sphere_has_its_zero_crossing_at_the_radius():
    """R = 32 over [-1, 1]^3 (h = 0.0625, tau = 4 h), a sphere of radius 0.6 seen by 6 axis-aligned cameras at distance 3
    (96 x 96, nearest-pixel lookup).  Measured on the reference: the vertices of the zero level set lie within 0.0247 of the
    radius (0.39 h; mean -0.0015).  Asserted: within h / 2 = 0.03125, the lattice's own resolution."""
    st, lo, hi, tau, *_ = T.sphere_fixture()
    assert tau == 0.25
    v, f, _ = M.marching_cubes(T.volume(st, 1), 0.0, lo, hi)
    assert len(v) > 1000 and M.closed_and_oriented(f)
    err = np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - 0.6)
    print("max radial error", err.max())
    assert err.max() < 0.03125
    assert abs(M.enclosed_volume(v, f) / (4.0 / 3.0 * np.pi * 0.6 ** 3) - 1.0) < 0.05


def test_depth_over_acc_of_the_teacher_is_distance_along_the_optical_axis():
    """The project's convention: z is the parameter of o + z d with d = R [(col - cx) / fx, -(row - cy) / fy, -1], so the
    compositor's depth = sum w z over acc = sum w is the axial distance of what the ray hits.  A camera at (0, 0, 4) looking
    down -z sees the base plate's top face (z = -0.35, perpendicular to the axis) at axial distance 4.35 in every pixel; the
    pixel towards (1.0, -0.6) has |d| = 1.035, so its Euclidean distance would be 4.50.  With sigma = 50 the weights are an
    exponential of mean 1 / (50 |d|) in z behind the face, sampled every dt: depth / acc lies in [4.35, 4.35 + 0.02 + 2 dt]."""
    from nerf_meets_mlx_amd.dataset import synthetic
    H = W = 64
    K, _ = synthetic.intrinsics(H, W)
    c2w = np.concatenate([np.eye(3), [[0.0], [0.0], [4.0]]], 1)
    axial = 4.0 - (-0.45 + 0.10)
    near, far, n = 4.0, 4.7, 7001
    dt = (far - near) / (n - 1)
    checked = 0
    for target in ((1.0, -0.6), (0.95, 0.6), (-1.0, -0.6), (0.0, -0.65)):               # on the plate, clear of every brick
        col = int(round(K[0, 2] + K[0, 0] * target[0] / axial))
        row = int(round(K[1, 2] - K[1, 1] * target[1] / axial))
        assert 0 <= col < W and 0 <= row < H
        d = c2w[:3, :3] @ np.array([(col - K[0, 2]) / K[0, 0], -(row - K[1, 2]) / K[1, 1], -1.0])
        z = torch.linspace(near, far, n, dtype=torch.float64)
        pts = torch.from_numpy(c2w[:3, 3]) + torch.from_numpy(d) * z[:, None]
        sigma, _ = synthetic.teacher_field(pts)
        delta = torch.cat([z[1:] - z[:-1], torch.tensor([1e10], dtype=torch.float64)]) * float(np.linalg.norm(d))
        alpha = 1.0 - torch.exp(-sigma * delta)
        Tr = torch.cumprod(torch.cat([torch.ones(1, dtype=torch.float64), 1.0 - alpha + 1e-10]), 0)[:-1]
        w = alpha * Tr
        acc, depth = float(w.sum()), float((w * z).sum())
        assert acc > 0.999
        got = depth / acc
        print(target, "depth / acc", got, "axial", axial, "euclidean", axial * np.linalg.norm(d))
        assert 0.0 <= got - axial <= 1.0 / 50.0 + 2 * dt
        if np.linalg.norm(d) > 1.02:
            assert axial * np.linalg.norm(d) - got > 0.05                                # not the Euclidean distance
            checked += 1
    assert checked >= 3
    # the analytic sphere maps of tests/_tsdf_ref.py follow the same convention: the pole under the central pixel
    depth_map, acc_map = T.sphere_maps(c2w, K, H, W, 0.6)
    cy, cx = H // 2, W // 2
    assert acc_map[cy * W + cx] == 1.0 and abs(depth_map[cy * W + cx] - 3.4) < 1e-5      # the pole at z = 0.6, axial 4 - 0.6


def test_finish_rule_three_branches():
    st = T.State(2)
    st.D[:] = np.array([0.5, -0.25, 0.75, 1.0, -1.0, 0.0, 0.3, -0.0], _F)
    st.Wt[:] = np.array([1, 2, 0, 0, 3, 1, 0, 2], _F)
    st.flags[:] = np.array([0, 1, 1, 0, 0, 1, 1, 0], np.uint8)
    v1 = T.volume(st, 1).reshape(-1)
    assert v1.dtype == _F and v1.tolist() == [-0.5, 0.25, 1.0, -1.0, 1.0, 0.0, 1.0, 0.0]
    assert np.signbit(v1[5]) == False and np.signbit(v1[7]) == False                     # 0.0f - (+-0) = +0
    v2 = T.volume(st, 2).reshape(-1)
    assert v2.tolist() == [-1.0, 0.25, 1.0, -1.0, 1.0, 1.0, 1.0, 0.0]
    assert (T.volume(T.State(3), 1) == -1.0).all()                                        # nothing fused: all outside


def test_plus_one_behind_a_surface_leaves_no_inner_shell():
    """Along the lattice line through the sphere's centre the volume changes sides twice: in at one side, out at the other.
    Without the occlusion flag the voxels deeper than tau are "never seen" = outside, and every surface has an inner twin."""
    st, lo, hi, tau, *_ = T.sphere_fixture()
    R = st.R
    crossings = lambda line: int((np.diff((line > 0).astype(np.int64)) != 0).sum())
    vol = T.volume(st, 1)
    for line in (vol[R // 2, R // 2, :], vol[R // 2, :, R // 2], vol[:, R // 2, R // 2]):
        assert crossings(line) == 2
    bare = st.copy()
    bare.flags[:] = 0
    assert crossings(T.volume(bare, 1)[R // 2, R // 2, :]) == 4
    # the whole mesh is one closed sheet: one component, Euler characteristic 2
    v, f, _ = M.marching_cubes(vol, 0.0, lo, hi)
    assert M.closed_and_oriented(f) and M.euler(v, f) == 2


def test_reference_batches_equal_single_views_and_carving_is_an_observation():
    st, lo, hi, tau, views, depth, acc, H, W = T.sphere_fixture(R=12, H=24, W=24)
    one = T.State(12)
    for s in range(len(views)):
        T.integrate(one, lo, hi, views[s:s + 1], H, W, depth[s:s + 1], acc[s:s + 1], tau, 0.5, 6.0, True)
    assert np.array_equal(one.D.view(np.uint32), st.D.view(np.uint32)) and np.array_equal(one.Wt, st.Wt)
    assert np.array_equal(one.flags, st.flags)
    nocarve = T.integrate(T.State(12), lo, hi, views, H, W, depth, acc, tau, 0.5, 6.0, False)
    assert (nocarve.Wt <= st.Wt).all() and (nocarve.Wt < st.Wt).any()
    near_far = T.integrate(T.State(12), lo, hi, views, H, W, depth, acc, tau, 0.5, 3.0, True)     # far in the middle of the box
    assert (near_far.Wt <= st.Wt).all() and (near_far.Wt < st.Wt).any() and (near_far.Wt >= nocarve.Wt).all()
