"""The mesh rasteriser on the GPU (csrc/raster.hip, engine/mesh/raster.py rasterize / render_mesh, Trainer.render_mesh / mesh_psnr)
against the numpy reference of tests/_raster_ref.py: keys, face, barycentrics, depth, acc, stats and the vertex-colour picture
compared as integers -- no tolerance, the rule is exact -- into sentinel-filled outputs with a spare row, the key buffer poisoned
before the clear; every small_max gives the same bits; face order and chunked draws change nothing; dropped faces are counted;
and the picture through a baked texture is the field's colour at the surface point each pixel sees."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _raster_ref as R
from tests import _smooth_ref as S
from tests import _texture_ref as T
from tests._poison import SENTINEL, bits_equal, poison_, sentinel_, unwritten

pytestmark = pytest.mark.gpu
DEV = "cuda"
NEAR = 0.01


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"


def _dev(a, dtype):
    return torch.from_numpy(np.array(a, order="C")).to(device=DEV, dtype=dtype).contiguous()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _soup():
    rng = np.random.default_rng(37)
    v = (rng.standard_normal((40, 3)) * [1.0, 0.8, 1.2] + S.CENTRE).astype(np.float32)
    f = np.stack([rng.permutation(40)[:3] for _ in range(37)]).astype(np.int32)
    return v, f


MESHES = {"tetrahedron": S.tetrahedron, "sphere12": lambda: S.sphere(12), "sphere24": lambda: S.sphere(24), "soup37": _soup}
# the whole mesh in view; and from nearby, looking past it, so that part of it lies outside the image
POSES = [R.look_at(S.CENTRE + [2.6, 1.1, 2.2], S.CENTRE), R.look_at(S.CENTRE + [-1.2, 0.4, 2.0], S.CENTRE + [0.9, 0.5, 0.0])]


def _view_ptr(view):
    return np.ascontiguousarray(view, np.float32).ctypes.data_as(C.POINTER(C.c_float))


class Buffers:
    """Keys with a spare row, poisoned; stats poisoned: the clear has to write both."""

    def __init__(self, H, W):
        self.H, self.W = H, W
        self.keys = poison_(torch.empty((H + 1) * W, dtype=torch.int64, device=DEV), 0xA5)
        self.stats = poison_(torch.empty(5, dtype=torch.int64, device=DEV), 0xA5)

    def clear(self):
        from nerf_meets_mlx_amd import _native as N
        N.check(N.lib().nerf_raster_clear(N.ptr(self.keys), self.H, self.W, N.ptr(self.stats), N.stream()))
        return self

    def draw(self, v, f, view, near=NEAR, cull=False, small_max=R.SMALL_MAX, base=0):
        from nerf_meets_mlx_amd import _native as N
        N.check(N.lib().nerf_raster_draw(N.ptr(v), v.shape[0], N.ptr(f), f.shape[0], base, _view_ptr(view), self.H, self.W, near, int(cull),
                                         small_max, N.ptr(self.keys), N.ptr(self.stats), N.stream()))
        return self

    def resolve(self, v, f, view, near=NEAR):
        from nerf_meets_mlx_amd import _native as N
        H, W = self.H, self.W
        face = sentinel_(torch.empty(H + 1, W, dtype=torch.int32, device=DEV))
        bary, depth, acc = (sentinel_(torch.empty(*s, dtype=torch.float32, device=DEV)) for s in ((H + 1, W, 2), (H + 1, W), (H + 1, W)))
        N.check(N.lib().nerf_raster_resolve(N.ptr(self.keys), N.ptr(v), v.shape[0], N.ptr(f), f.shape[0], _view_ptr(view), H, W, near,
                                            N.ptr(face), N.ptr(bary), N.ptr(depth), N.ptr(acc), N.stream()))
        assert bool((face[H:] == SENTINEL).all()) and not bool((face[:H] == SENTINEL).any())
        for t in (bary, depth, acc):
            assert unwritten(t[H:]) == t[H:].numel() and unwritten(t[:H]) == 0
        return face[:H], bary[:H], depth[:H], acc[:H]

    def host(self):
        """(keys uint64 [H W], stats uint64 [4]); the spare row and the spare stats word still hold the poison."""
        n = self.H * self.W
        k = self.keys.cpu().numpy().view(np.uint64)
        s = self.stats.cpu().numpy().view(np.uint64)
        assert (k[n:] == np.uint64(0xA5A5A5A5A5A5A5A5)).all() and s[4] == np.uint64(0xA5A5A5A5A5A5A5A5)
        return k[:n].copy(), s[:4].copy()


def _shade(face, bary, f, V, H, W, colors=None, rgb_in=None, background=None, per_pixel=0):
    from nerf_meets_mlx_amd import _native as N
    rgb = sentinel_(torch.empty(H + 1, W, 3, dtype=torch.float32, device=DEV))
    N.check(N.lib().nerf_raster_shade(N.ptr(face), N.ptr(bary), N.ptr(f), V, f.shape[0], N.ptr(colors), N.ptr(rgb_in), N.ptr(background),
                                      per_pixel, H, W, N.ptr(rgb), N.stream()))
    assert unwritten(rgb[H:]) == 3 * W and unwritten(rgb[:H]) == 0
    return rgb[:H]


def _same(got, want, what):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    bad = np.nonzero(got != want)[0]
    assert got.shape == want.shape and len(bad) == 0, (what, len(bad), bad[:4], got[bad[:4]], want[bad[:4]])


def _check_against_reference(v, f, view, H, W, near=NEAR, cull=False, small_max=R.SMALL_MAX, colors=None):
    """One cleared draw, resolved (and shaded with vertex colours): every output equals the reference's as integers."""
    want = R.render(v, f, view, H, W, near, cull)
    dv, df = _dev(v, torch.float32), _dev(f, torch.int32)
    buf = Buffers(H, W).clear().draw(dv, df, view, near, cull, small_max)
    keys, stats = buf.host()
    _same(keys, want[0], "keys")
    _same(stats, want[1], "stats")
    face, bary, depth, acc = buf.resolve(dv, df, view, near)
    _same(face.cpu().numpy(), want[2], "face")
    for name, g, w in (("bary", bary, want[3]), ("depth", depth, want[4]), ("acc", acc, want[5])):
        _same(_bits(g.cpu().numpy()), _bits(w), name)
    if colors is not None:
        bg = np.array([0.25, 0.5, 0.75], np.float32)
        rgb = _shade(face, bary, df, len(v), H, W, colors=_dev(colors, torch.float32), background=_dev(bg, torch.float32))
        _same(_bits(rgb.cpu().numpy()), _bits(R.shade(want[2], want[3], f, len(v), bg, colors=colors)), "rgb")
    return want, (keys, stats, face, bary, depth, acc)


# ------------------------------------------------------------------------------------------------ bits
@pytest.mark.parametrize("pose", [0, 1])
@pytest.mark.parametrize("name,H,W", [("tetrahedron", 48, 64), ("sphere12", 48, 64), ("sphere24", 17, 33), ("sphere24", 96, 96),
                                      ("soup37", 48, 64)])
def test_every_output_matches_the_reference_bit_for_bit(name, H, W, pose):
    v, f = MESHES[name]()
    view = R.view_of(POSES[pose], R.intrinsics(H, W))
    colors = np.random.default_rng(len(f)).uniform(0, 1, (len(v), 3)).astype(np.float32)
    want, _ = _check_against_reference(v, f, view, H, W, colors=colors)
    stats, acc = want[1], want[5]
    print(name, H, W, "pose", pose, "stats", stats, "covered", int(acc.sum()))
    assert 0 < acc.sum() < H * W and stats[3] > acc.sum()                # something is seen, something is not, something is hidden
    x0, x1, y0, y1 = R.boxes(*R.setup(v, f, view, NEAR)[1:3], H, W)
    n = ((x1 - x0 + 1) * (y1 - y0 + 1))[(x0 <= x1) & (y0 <= y1)]
    if name == "tetrahedron":
        assert n.min() > 100                                             # hundreds of pixels a face: the cooperative path
    if name == "sphere24":
        assert (n <= R.SMALL_MAX).sum() > 500                            # the per-lane path
    if pose == 1:                                                        # part of the mesh lies outside the image
        u, w, _ = R.project(v[f.reshape(-1)], view)
        assert ((u < 0) | (u > W - 1) | (w < 0) | (w > H - 1)).any()


# ------------------------------------------------------------------------------------------------ small_max
def _fan_scene(H, W):
    c2w, K = R.look_at([0.0, 0.0, 0.0], [0.0, 0.0, -1.0]), R.intrinsics(H, W)
    sizes = []
    for k, n in enumerate([1, 2, 3, 4, 5, 15, 16, 17]):                  # small_max - 1, small_max, small_max + 1 for 1, 4, 16 (and 2)
        sizes.append((3 + (k % 2) * 20, 2 + 4 * k, n, 1))                # n x 1, inside the image
        sizes.append((-3, 3 + 4 * k, n + 3, 1))                          # clipped to n x 1 by the left edge
    sizes += [(45, 2, 4, 4), (45, 8, 1, 17), (45, 27, 5, 3), (52, 2, 8, 2), (W - 2, 30, 5, 8), (50, H - 2, 8, 4)]
    v, f = R.fan(c2w, K, sizes)
    return v, f, R.view_of(c2w, K)


def test_small_max_does_not_change_a_bit():
    H, W = 40, 64
    v, f, view = _fan_scene(H, W)
    why, X, Y, _, _ = R.setup(v, f, view, NEAR)
    x0, x1, y0, y1 = R.boxes(X, Y, H, W)
    n = (x1 - x0 + 1) * (y1 - y0 + 1)
    assert (why == R.OK).all() and list(n[:16:2]) == [1, 2, 3, 4, 5, 15, 16, 17] == list(n[1:16:2])
    assert list(n[16:]) == [16, 17, 15, 16, 16, 16]
    v2, f2 = S.sphere(24)
    view2 = R.view_of(POSES[0], R.intrinsics(H, W))
    for verts, faces, vw in ((v, f, view), (v2, f2, view2)):
        first = None
        for sm in (0, 1, 4, R.SMALL_MAX, 1 << 30):
            _, got = _check_against_reference(verts, faces, vw, H, W, small_max=sm)
            if first is None:
                first = got
            _same(got[0], first[0], ("keys", sm))
            _same(got[1], first[1], ("stats", sm))
            for a, b in zip(got[2:], first[2:]):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), sm


# ------------------------------------------------------------------------------------------------ stability
def test_runs_face_order_and_chunks_agree():
    H, W = 48, 64
    v, f = S.sphere(24)
    view = R.view_of(POSES[1], R.intrinsics(H, W))
    dv, df = _dev(v, torch.float32), _dev(f, torch.int32)
    one = Buffers(H, W).clear().draw(dv, df, view)
    keys, stats = one.host()
    again = Buffers(H, W).clear().draw(dv, df, view).host()
    _same(again[0], keys, "second run")
    _same(again[1], stats, "second run")
    # two chunks of faces into one buffer, the second with its ids offset (and drawn first): the same keys, the same stats
    k = 1234
    two = Buffers(H, W).clear().draw(dv, df[k:].contiguous(), view, base=k).draw(dv, df[:k].contiguous(), view)
    _same(two.host()[0], keys, "chunks")
    _same(two.host()[1], stats, "chunks")
    for a, b in zip(two.resolve(dv, df, view), one.resolve(dv, df, view)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # a permutation of the faces: the same depth and mask; the same face wherever the winning depth is unique
    perm = np.random.default_rng(3).permutation(len(f))
    dp = _dev(f[perm], torch.int32)
    pk, ps = Buffers(H, W).clear().draw(dv, dp, view).host()
    _same(pk >> np.uint64(32), keys >> np.uint64(32), "depth bits under a permutation")
    _same(ps, stats, "stats under a permutation")
    want = R.render(v, f, view, H, W, NEAR)
    face = want[2]
    # unique: no other face covers the pixel at the same depth -- count the (pixel, face) pairs at the winning depth
    why, X, Y, z, s = R.setup(v, f, view, NEAR)
    ties = np.zeros(H * W, np.int64)
    py, px = np.mgrid[0:H, 0:W]
    for j in np.nonzero(why == R.OK)[0]:
        cov, _, _, d = R.pixel(X[j], Y[j], z[j], s[j], px, py)
        ties += (cov & (_bits(d) == _bits(want[4]).reshape(H, W))).reshape(-1)
    unique = (face >= 0) & (ties == 1)
    assert unique.sum() > 0.9 * (face >= 0).sum()
    got = (pk & np.uint64(0xFFFFFFFF)).astype(np.int64)
    _same(perm[got[unique]], face[unique], "face through the permutation")


# ------------------------------------------------------------------------------------------------ dropped faces, tiny images
def test_dropped_faces_are_counted_and_leave_no_key():
    H, W = 48, 64
    c2w = POSES[0]
    view = R.view_of(c2w, R.intrinsics(H, W))
    v0, f0 = S.sphere(12)
    near = 0.25
    v, f, n_depth, n_other = R.drop_scene(c2w, v0, f0[:101], near)
    assert len(f) == 101                                                  # the last wave is partial
    why0 = R.setup(v0, f0[:101], view, near)[0]
    why = R.setup(v, f, view, near)[0]
    assert list(why[[1, 3, 5]]) == [R.DROP_DEPTH] * 3 and list(why[[7, 9, 11, 13, 15, 17, 100]]) == [R.DROP_OTHER] * 7
    assert (why0 == R.OK).all() and (why == R.OK).sum() == 101 - n_depth - n_other
    want, _ = _check_against_reference(v, f, view, H, W, near=near)
    assert list(want[1][:3]) == [101 - n_depth - n_other, n_depth, n_other]
    assert not np.isin(want[2], [1, 3, 5, 7, 9, 11, 13, 15, 17, 100]).any() and (want[2] >= 0).any()
    want, _ = _check_against_reference(v, f, view, H, W, near=near, cull=True)
    assert want[1][0] < 101 - n_depth - n_other and want[1][:3].sum() == 101
    # every face dropped: an empty picture
    all_bad = np.full((70, 3), len(v), np.int32)
    want, got = _check_against_reference(v, all_bad, view, H, W)
    assert list(want[1]) == [0, 0, 70, 0] and bool((got[2] == -1).all()) and not bool(got[4].any())


@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (9, 1)])
def test_images_of_one_row_or_column(H, W):
    v, f = S.tetrahedron()
    K = np.array([[8.0, 0.0, 0.5 * (W - 1)], [0.0, 8.0, 0.5 * (H - 1)], [0.0, 0.0, 1.0]])
    want, _ = _check_against_reference(v, f, R.view_of(POSES[0], K), H, W)
    assert want[5].any()


def test_no_faces_on_the_device():
    from nerf_meets_mlx_amd.engine import mesh as E
    v = _dev(S.tetrahedron()[0], torch.float32)
    m = E.Mesh(v, torch.zeros(0, 3, dtype=torch.int32, device=DEV), torch.zeros_like(v), torch.zeros_like(v))
    bg = torch.rand(5 * 6, 3, device=DEV)
    fr = E.render_mesh(m, POSES[0], R.intrinsics(5, 6), 5, 6, background=bg)
    assert fr.rgb.is_cuda and bits_equal(fr.rgb, bg.reshape(5, 6, 3)) and bool((fr.face == -1).all()) and not fr.acc.any()
    face, bary, depth, acc, stats = E.rasterize(m, POSES[0], R.intrinsics(5, 6), 5, 6)
    assert stats.tolist() == [0, 0, 0, 0] and face.shape == (5, 6) and bary.shape == (5, 6, 2) and not depth.any()


# ------------------------------------------------------------------------------------------------ engine, texture
AFFINE_M = np.array([[0.1, 0.05, -0.08], [-0.06, 0.1, 0.07], [0.04, -0.09, 0.1]])
AFFINE_C = np.array([0.5, 0.42, 0.3])


def test_engine_equals_the_entries_and_the_reference():
    from nerf_meets_mlx_amd.engine import mesh as E
    H, W = 48, 64
    v, f = S.sphere(12)
    K = R.intrinsics(H, W)
    colors = np.random.default_rng(1).uniform(0, 1, (len(v), 3)).astype(np.float32)
    mesh = E.Mesh(_dev(v, torch.float32), _dev(f, torch.int32), _dev(T.vertex_normals(v, f), torch.float32), _dev(colors, torch.float32))
    want = R.render(v, f, R.view_of(POSES[0], K), H, W, E.RASTER_NEAR)
    stages = []
    fr = E.render_mesh(mesh, torch.from_numpy(POSES[0]), torch.from_numpy(K), H, W, mark=stages.append)
    assert stages == ["clear", "draw", "resolve", "shade"] and isinstance(fr, E.MeshFrame)
    assert fr.rgb.shape == (H, W, 3) and fr.depth.shape == (H, W) and fr.face.dtype == torch.int32 and fr.bary.shape == (H, W, 2)
    _same(fr.face.cpu().numpy(), want[2], "face")
    _same(_bits(fr.depth.cpu().numpy()), _bits(want[4]), "depth")
    _same(_bits(fr.rgb.cpu().numpy()), _bits(R.shade(want[2], want[3], f, len(v), np.ones(3, np.float32), colors=colors)), "rgb on white")
    face, bary, depth, acc, stats = E.rasterize(mesh, POSES[0], K, H, W, cull_backfaces=True, small_max=0)
    assert torch.equal(face, fr.face) and bits_equal(bary, fr.bary) and bits_equal(depth, fr.depth) and bits_equal(acc, fr.acc)
    _same(stats.cpu().numpy().view(np.uint64), R.render(v, f, R.view_of(POSES[0], K), H, W, E.RASTER_NEAR, cull=True)[1], "stats")
    with pytest.raises(ValueError, match="needs a texture"):
        E.render_mesh(mesh._replace(colors=None), POSES[0], K, H, W)


@pytest.mark.parametrize("per_pixel", [False, True])
def test_the_picture_through_a_texture_is_the_field_at_the_surface(per_pixel):
    """sphere24 with its faces permuted, the affine colour of tests/test_gpu_texture.py baked at T = 8: on every covered pixel the
    lookup at the pixel's (face, bary) is within that test's bound 0.5 / 255 + 1e-5 of the colour at the reconstructed surface
    point; empty pixels are exactly the background."""
    from nerf_meets_mlx_amd.engine import mesh as E
    H, W = 96, 96
    v, f = S.sphere(24)
    f = f[np.random.default_rng(24).permutation(len(f))]
    mesh = E.Mesh(_dev(v, torch.float32), _dev(f, torch.int32), _dev(T.vertex_normals(v, f), torch.float32))
    M32, c32 = _dev(AFFINE_M, torch.float32), _dev(AFFINE_C, torch.float32)

    def query(rows, z):
        raw = torch.ones(rows.shape[0], 1, 4, dtype=torch.float32, device=rows.device)
        raw[:, 0, :3] = rows[:, :3] @ M32.T + c32
        return raw
    tex = E.bake_texture(query, mesh, 8)
    K = R.intrinsics(H, W)
    bg = torch.rand(H * W, 3, device=DEV) if per_pixel else torch.tensor([0.125, 0.5, 0.875], device=DEV)
    stages = []
    fr = E.render_mesh(mesh, POSES[0], K, H, W, texture=tex, background=bg, mark=stages.append)
    assert stages == ["clear", "draw", "resolve", "texture", "shade"]
    hit = (fr.face >= 0).cpu().numpy()
    assert 500 < hit.sum() < H * W - 500 and np.array_equal(hit, fr.acc.cpu().numpy() == 1.0)
    face, bary = fr.face.cpu().numpy()[hit].astype(np.int64), fr.bary.cpu().numpy()[hit].astype(np.float64)
    A, B, Cc = (v[f[face, k]].astype(np.float64) for k in range(3))
    point = (1.0 - bary[:, :1] - bary[:, 1:]) * A + bary[:, :1] * B + bary[:, 1:] * Cc
    want = point @ AFFINE_M.T + AFFINE_C
    err = np.abs(fr.rgb.cpu().numpy()[hit].astype(np.float64) - want).max()
    print("covered", int(hit.sum()), "max |picture - field|", err, "bound", 0.5 / 255 + 1e-5)
    assert err <= 0.5 / 255 + 1e-5
    empty = torch.from_numpy(~hit).to(DEV)
    bgp = bg.reshape(H, W, 3) if per_pixel else bg.expand(H, W, 3)
    assert bits_equal(fr.rgb[empty], bgp[empty])
    # the surface point is the one the pixel's ray hits: it projects back to the pixel centre, at the frame's depth
    u, w, zc = R.project(point.astype(np.float32), R.view_of(POSES[0], K))
    py, px = np.nonzero(hit)
    assert np.abs(u - px).max() < 0.02 and np.abs(w - py).max() < 0.02 and np.abs(zc - fr.depth.cpu().numpy()[hit]).max() < 1e-4


# ------------------------------------------------------------------------------------------------ trainer
def test_trainer_render_mesh_and_mesh_psnr():
    from nerf_meets_mlx_amd.dataset import synthetic
    from nerf_meets_mlx_amd.engine import mesh as E
    from nerf_meets_mlx_amd.engine.trainer import Trainer
    imgs, poses, _, _, K = synthetic.make_dataset(8, 8, 2, seed=0, device=DEV)
    tr = Trainer(imgs, poses, K, N_rand=64, n_depth_samples=16, N_importance=16, seed=4, device=DEV)
    box = ([-1.0] * 3, [1.0] * 3)
    vol = tr.density_volume(16, box)
    m = tr.extract_mesh(resolution=16, threshold=float(vol.reshape(-1).quantile(0.7)), aabb=box)
    assert m.faces.shape[0] > 0 and m.colors is not None
    c2w = poses[0].cpu().numpy() if torch.is_tensor(poses) else np.asarray(poses[0])
    fr = tr.render_mesh(m, c2w)
    want = E.render_mesh(m, c2w, tr.K, tr.H, tr.W, near=float(tr.near))
    for a, b in zip(fr, want):
        assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert fr.rgb.shape == (8, 8, 3)
    tex = tr.texture_mesh(m, texels=4)
    bg = torch.tensor([0.2, 0.3, 0.4], device=DEV)
    ft = tr.render_mesh(m, c2w, texture=tex, background=bg)
    wt = E.render_mesh(m, c2w, tr.K, tr.H, tr.W, texture=tex, background=bg, near=float(tr.near))
    assert bits_equal(ft.rgb, wt.rgb) and torch.equal(ft.face, fr.face)
    gt = imgs[0][..., :3].to(DEV).float()
    for kw, frame in (({}, fr), ({"texture": tex, "background": bg}, ft)):
        mse = torch.mean((frame.rgb - gt) ** 2)
        assert tr.mesh_psnr(m, c2w, gt, **kw) == float(10.0 * torch.log10(1.0 / mse))
    # the frame's maps are a renderer's aux maps: TSDF fusion takes them as they are
    tsdf = E.TSDFVolume(16, box[0], box[1])
    tsdf.integrate(fr.depth, fr.acc, c2w, tr.K, tr.H, tr.W, far=float(tr.far))
    assert tsdf.volume().shape == (16, 16, 16) and bool(torch.isfinite(tsdf.D).all())
