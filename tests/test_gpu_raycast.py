"""Mesh ray casting on the GPU (csrc/raycast.hip, engine/mesh/raycast.py) against the numpy mirror of tests/_raycast_ref.py, which
tests/test_raycast_host.py holds to the scan over every face: t, face, bary and visits compared as integer bit patterns -- no
tolerance, the rule is exact and every operation (the float64 division and the casts to float32 among them) is correctly rounded on
both sides -- into sentinel-filled outputs that carry one spare row, with a poisoned hierarchy workspace; then the engine: chunks,
sorted casts, a permuted face list, occlusion, visibility, the ray-cast frame, its shading, and the depth error against a field."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _distance_ref as D
from tests import _raster_ref as R
from tests import _raycast_ref as RC
from tests._poison import BIG_BYTES, NAN_BYTES, SENTINEL, bits_equal, poison_, sentinel_, unwritten

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"


def _dev(a, dtype):
    return torch.from_numpy(np.array(a, order="C")).to(device=DEV, dtype=dtype).contiguous()


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


def _mesh(v, f, colors=None):
    from nerf_meets_mlx_amd.engine import mesh as E
    tv = _dev(v, torch.float32).reshape(-1, 3)
    return E.Mesh(tv, _dev(f, torch.int32).reshape(-1, 3), torch.zeros_like(tv), colors)


class _Tree:
    """nerf_bvh_keys / torch.sort / nerf_bvh_build on numpy inputs with a poisoned workspace; cast() and any() are the two C calls
    of csrc/raycast.hip into sentinel outputs with one spare row, with the workspace and the inputs compared before and after."""

    def __init__(self, v, f, pattern=NAN_BYTES, lo=D.LO, hi=D.HI):
        from nerf_meets_mlx_amd import _native as N
        self.N, self.L = N, N.lib()
        self.v0, self.f0 = np.array(v, F32).reshape(-1, 3), np.array(f, np.int32).reshape(-1, 3)
        self.tv, self.tf = _dev(self.v0, torch.float32), _dev(self.f0, torch.int32)
        self.V, self.F = len(self.v0), len(self.f0)
        self.box = ((C.c_float * 3)(*lo), (C.c_float * 3)(*hi))
        self.ws = poison_(torch.empty(self.L.nerf_bvh_workspace_bytes(self.F), dtype=torch.uint8, device=DEV), pattern)
        keys = torch.empty(self.F, dtype=torch.int64, device=DEV)
        N.check(self.L.nerf_bvh_keys(N.ptr(self.tv), self.V, N.ptr(self.tf), self.F, *self.box, N.ptr(keys), N.stream()))
        skeys = torch.sort(keys).values.contiguous()
        N.check(self.L.nerf_bvh_build(N.ptr(self.tv), self.V, N.ptr(self.tf), self.F, N.ptr(skeys), N.ptr(self.ws), N.stream()))
        torch.cuda.synchronize()

    def _call(self, fn, rays, outs):
        N, n = self.N, len(rays)
        r0 = np.asarray(rays, F32).reshape(-1, RC.STRIDE)
        tr = _dev(r0, torch.float32)
        before = self.ws.clone()
        N.check(fn(N.ptr(tr), n, N.ptr(self.tv), self.V, N.ptr(self.tf), self.F, *self.box, N.ptr(self.ws), *(N.ptr(o) for o in outs),
                   N.stream()))
        torch.cuda.synchronize()
        assert torch.equal(before, self.ws)                            # the hierarchy is only read
        assert np.array_equal(_bits(tr.cpu().numpy()), _bits(r0))
        assert np.array_equal(_bits(self.tv.cpu().numpy()), _bits(self.v0)) and np.array_equal(self.tf.cpu().numpy(), self.f0)

    def cast(self, rays):
        n = len(rays)
        t = sentinel_(torch.empty(n + 1, dtype=torch.float32, device=DEV))
        face = torch.full((n + 1,), SENTINEL, dtype=torch.int32, device=DEV)
        bary = sentinel_(torch.empty(n + 1, 2, dtype=torch.float32, device=DEV))
        visits = torch.full((n + 1, 2), SENTINEL, dtype=torch.int32, device=DEV)
        self._call(self.L.nerf_raycast, rays, (t, face, bary, visits))
        assert unwritten(t[n:]) == 1 and int(face[n]) == SENTINEL and unwritten(bary[n:]) == 2 and (visits[n] == SENTINEL).all()
        assert unwritten(t[:n]) == 0 and unwritten(bary[:n]) == 0 and not bool((face[:n] == SENTINEL).any())
        assert not bool((visits[:n] == SENTINEL).any())
        return tuple(x[:n].cpu().numpy() for x in (t, face, bary, visits))

    def any(self, rays):
        n = len(rays)
        hit = torch.full((n + 1,), 0xA5, dtype=torch.uint8, device=DEV)
        self._call(self.L.nerf_raycast_any, rays, (hit,))
        assert int(hit[n]) == 0xA5
        return hit[:n].cpu().numpy()


def _assert_same(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        bad = (_bits(g) != _bits(w)) if g.dtype == F32 else (g != w)
        assert not bad.any(), (what, ("t", "face", "bary", "visits")[k], int(bad.sum()), np.nonzero(bad)[0][:6], g[bad][:6], w[bad][:6])


# ------------------------------------------------------------------------------------------------ against the mirror
@pytest.mark.parametrize("name", sorted(RC.MESHES))
def test_cast_matches_the_mirror_bit_for_bit(name):
    v, f, rays, brute, walk, hit = RC.case(name)
    for pattern in (NAN_BYTES, BIG_BYTES):
        t = _Tree(v, f, pattern)
        _assert_same(t.cast(rays), walk, (name, pattern))              # t, face, bary and the two counters
        assert np.array_equal(t.any(rays), hit), (name, pattern)
    _assert_same(walk[:3], brute, name)                                # and so the scan over every face
    assert np.array_equal(hit != 0, walk[1] >= 0)


def test_ragged_chunks_repeats_and_sorted_casts():
    from nerf_meets_mlx_amd.engine import mesh as E
    v, f, rays, brute, walk, hit = RC.case("sphere24")
    t = _Tree(v, f)
    first = t.cast(rays)
    _assert_same(t.cast(rays), first, "repeat")
    a, b, c = t.cast(rays[:100]), t.cast(rays[100:101]), t.cast(rays[101:])          # three ragged chunks against one tree
    _assert_same(tuple(np.concatenate(x) for x in zip(a, b, c)), first, "chunks")
    m, tr = _mesh(v, f), _dev(rays, torch.float32)
    caster = E.MeshRaycast(m, D.LO, D.HI)
    own = E.MeshRaycast(m, D.LO, D.HI, bvh=E.MeshBVH(m, D.LO, D.HI))
    for sort in (False, True, None):
        for cst in (caster, own):
            h = cst.cast(tr, sort=sort)
            assert isinstance(h, E.RayHits) and h.t.shape == (len(rays),) and h.bary.shape == h.visits.shape == (len(rays), 2)
            _assert_same(tuple(x.cpu().numpy() for x in h), walk, ("engine", sort))
            occ = cst.occluded(tr, sort=sort)
            assert occ.dtype == torch.bool and torch.equal(occ, h.face >= 0)
    e = caster.cast(tr[:0])
    assert e.t.shape == (0,) and e.face.dtype == torch.int32 and e.bary.shape == (0, 2) and caster.occluded(tr[:0]).shape == (0,)
    for bad in (tr.double(), tr.cpu(), tr[:, :8].contiguous()):
        with pytest.raises(ValueError, match="rays"):
            caster.cast(bad)
        with pytest.raises(ValueError, match="rays"):
            caster.occluded(bad)
    empty = E.MeshRaycast(_mesh(v, np.zeros((0, 3), np.int32)), D.LO, D.HI)
    h = empty.cast(tr)
    good = RC.valid_rays(rays)
    assert empty.P == 1 and np.isposinf(h.t.cpu().numpy()[good]).all() and bool((h.face == -1).all())
    assert bool((h.visits.cpu()[torch.from_numpy(good)] == torch.tensor([0, 1], dtype=torch.int32)).all())


def test_a_permuted_face_list_moves_the_face_and_nothing_else():
    v, f, rays, brute, walk, _ = RC.case("sphere24")
    perm = np.random.default_rng(9).permutation(len(f))
    pt, pf, pb, _ = _Tree(v, f[perm], BIG_BYTES).cast(rays)
    t, face, bary = brute
    assert np.array_equal(_bits(pt), _bits(t))                         # the same t under a renumbering
    hit = face >= 0
    assert np.array_equal(pf >= 0, hit)
    moved = perm[pf[hit]]
    # the face follows the permutation, up to ties in t (a ray through a shared edge): there the face answered attains the t
    tied = moved != face[hit]
    assert not tied.all()
    assert np.array_equal(_bits(pb[hit][~tied]), _bits(bary[hit][~tied]))
    bt, bf, bb = RC.brute_force(rays, v, f[perm])
    assert np.array_equal(pf, bf) and np.array_equal(_bits(pt), _bits(bt)) and np.array_equal(_bits(pb), _bits(bb))


def test_visible_on_the_cube():
    from nerf_meets_mlx_amd.engine import mesh as E
    v, f = D.cube()                                                    # [-0.5, 0.5]^3 + (0, 0.75, 1.5)
    caster = E.MeshRaycast(_mesh(v, f), D.LO, D.HI)
    on_right = _dev([[0.5, 0.875, 1.625]] * 4, torch.float32)          # a point on the side x = +0.5
    eyes = _dev([[3.0, 1.0, 2.0],                                      # outside that side: seen
                 [-3.0, 0.875, 1.625],                                 # behind the opposite side: the cube is in between
                 [0.25, 0.875, 1.625],                                 # inside the cube: nothing in between
                 [0.5, 0.875, 1.625]], torch.float32)                  # the point itself
    eps = 2.0 ** -10
    assert caster.visible(on_right, eyes, eps).tolist() == [True, False, True, True]
    assert caster.visible(on_right, eyes[0], eps).tolist() == [True] * 4           # one eye for all
    assert caster.visible(on_right[:2], eyes[:2], 0.0).tolist() == [False, False]  # without the margin the point's own side is hit
    for bad in (-1.0, float("nan"), None):
        with pytest.raises(ValueError, match="eps"):
            caster.visible(on_right, eyes, bad)
    with pytest.raises(ValueError, match="eyes"):
        caster.visible(on_right, eyes[:2], eps)


# ------------------------------------------------------------------------------------------------ frames
def test_raycast_frame_matches_the_mirror():
    from nerf_meets_mlx_amd.engine import mesh as E
    H = W = 64
    v, f, c2w, K, want = RC.sphere24_frame()
    m = _mesh(v, f)
    for kw in ({}, {"chunk": 1000}, {"caster": E.MeshRaycast(m, *RC.bounds(v))}):
        got = E.raycast_frame(m, c2w, K, H, W, **kw)
        assert [tuple(x.shape) for x in got] == [(H, W), (H, W, 2), (H, W), (H, W), (H, W, 2)]
        assert [x.dtype for x in got] == [torch.int32, torch.float32, torch.float32, torch.float32, torch.int32]
        for k, (g, w) in enumerate(zip(got, want)):
            g = g.cpu().numpy()
            assert np.array_equal(_bits(g) if g.dtype == F32 else g, _bits(w) if w.dtype == F32 else w), (kw.keys(), k)
    # far in front of the sphere: nothing is hit, and the frame is the empty one
    face, bary, depth, acc, _ = E.raycast_frame(m, c2w, K, H, W, far=0.5)
    assert bool((face == -1).all()) and not bool(bary.any()) and not bool(depth.any()) and not bool(acc.any())


def test_render_mesh_rays_shades_like_render_mesh():
    from nerf_meets_mlx_amd.engine import mesh as E
    H = W = 64
    v, f, c2w, K, want = RC.sphere24_frame()
    col = _dev(np.random.default_rng(3).random((len(v), 3)), torch.float32)
    m = _mesh(v, f, col)
    bg = [0.25, 0.5, 0.75]
    a, b = E.render_mesh_rays(m, c2w, K, H, W, background=bg), E.render_mesh(m, c2w, K, H, W, background=bg)
    assert isinstance(a, E.MeshFrame) and [tuple(x.shape) for x in a] == [tuple(x.shape) for x in b]
    assert [x.dtype for x in a] == [x.dtype for x in b]
    assert np.array_equal(a.face.cpu().numpy(), want[0]) and bits_equal(a.depth, torch.from_numpy(want[2].copy()).to(DEV))
    same = (a.face == b.face) & (a.face >= 0)
    assert int(same.sum()) > 1000
    # the shading's own float32 rounding: rgb = (wa ca + wb cb) + wc cc with colours in [0, 1] and wa = (1 - wb) - wc, so rgb moves
    # by at most twice the change of the two weights (each enters as itself and through wa), plus the roundings of either side:
    # two in wa, three products and two sums of numbers that stay below 2, at most 8 2^-24 a side
    dw = (a.bary.double() - b.bary.double()).abs().sum(-1)[same]
    drgb = (a.rgb.double() - b.rgb.double()).abs().max(-1).values[same]
    assert bool((drgb <= 2.0 * dw + 16 * 2.0 ** -24).all()), float((drgb - 2.0 * dw).max())
    empty = (a.face < 0) & (b.face < 0)
    assert bool((a.rgb[empty] == torch.tensor(bg, device=DEV)).all()) and bool((b.rgb[empty] == a.rgb[empty]).all())
    # shading the rays' own (face, bary) is the mirror's shade of them, bit for bit
    ref = R.shade(want[0].reshape(-1), want[1].reshape(-1, 2), f, len(v), np.array(bg, F32), col.cpu().numpy())
    assert np.array_equal(_bits(a.rgb.cpu().numpy().reshape(-1, 3)), _bits(ref))


def test_trainer_raycast_mesh_and_mesh_depth_error():
    """hw 48, march mode, 50 iterations, R = 32 (the field of tests/test_gpu_tsdf.py): keys, finiteness, the shares."""
    from nerf_meets_mlx_amd.dataset import synthetic
    from nerf_meets_mlx_amd.engine import mesh as E
    from nerf_meets_mlx_amd.engine.ngp import NGPTrainer
    imgs, poses, _, _, K = synthetic.make_dataset(48, 48, 8, seed=0, device=DEV)
    tr = NGPTrainer(imgs, poses, K, N_rand=1024, n_depth_samples=64, seed=4, device=DEV, log2_hashmap_size=14,
                    occupancy_grid=True, march_steps=1024)
    for _ in range(50):
        tr.train_step()
    m = tr.extract_mesh_tsdf(resolution=32)
    assert m.faces.shape[0] > 0
    err = tr.mesh_depth_error(m, poses[0])
    print("mesh_depth_error", err)
    assert sorted(err) == ["both", "field_only", "h", "mean", "mesh_only", "neither", "rms"]
    assert all(np.isfinite(x) for x in err.values())
    assert abs(err["both"] + err["mesh_only"] + err["field_only"] + err["neither"] - 1.0) < 1e-12
    assert err["both"] > 0 and 0.0 <= err["mean"] <= err["rms"] and err["h"] == 2.0 * float(tr.field.bound) / 256
    assert tr.mesh_depth_error(m, poses[0], resolution=128)["h"] == 2.0 * err["h"]
    for bad in (0.0, 1.5, None, True):
        with pytest.raises(ValueError, match="acc_min"):
            tr.mesh_depth_error(m, poses[0], acc_min=bad)
    fr = tr.raycast_mesh(m, poses[0])
    assert isinstance(fr, E.MeshFrame) and fr.rgb.shape == (48, 48, 3) and fr.face.dtype == torch.int32
    face, bary, depth, acc, _ = E.raycast_frame(m, poses[0], tr.K, 48, 48, near=float(tr.near), far=float(tr.far))
    assert torch.equal(fr.face, face) and bits_equal(fr.depth, depth) and bits_equal(fr.acc, acc) and bits_equal(fr.bary, bary)
    assert abs(float(acc.double().mean()) - (err["both"] + err["mesh_only"])) < 1e-12
