"""The projective texture bake on the GPU (csrc/project.hip, engine/mesh/project.py project_texture, Trainer.project_texture) against the
numpy reference of tests/_project_ref.py: state, image and seen compared as integers -- no tolerance, the rule is exact -- into
sentinel-filled outputs with a spare row; chunks, repeats and the split of the views over launches change no bit; NaN maps and
images, bad faces, texels outside the image or behind the near plane, the smallest images, no faces and no views; and end to end
through the engine's own rasterised maps, the mesh renderer, the OBJ writer and the trainer."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from tests import _project_ref as P
from tests import _raster_ref as R
from tests import _smooth_ref as S
from tests import _texture_ref as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
NEAR, TOL, COS_MIN, ACC_MIN = 0.01, 0.05, 0.1, 0.5
F32 = np.float32
POISON = 0xA5


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"


def _dev(a, dtype):
    return torch.from_numpy(np.array(a, order="C")).to(device=DEV, dtype=dtype).contiguous()


def _soup():
    rng = np.random.default_rng(37)
    v = (rng.standard_normal((40, 3)) * [1.0, 0.8, 1.2] + S.CENTRE).astype(F32)
    f = np.stack([rng.permutation(40)[:3] for _ in range(37)]).astype(np.int32)
    return v, f


def _sphere24_permuted():
    v, f = S.sphere(24)
    return v, f[np.random.default_rng(24).permutation(len(f))]


MESHES = {"tetrahedron": S.tetrahedron, "sphere12": lambda: S.sphere(12), "sphere24": _sphere24_permuted, "soup37": _soup}


def _mesh(name):
    v, f = MESHES[name]()
    return np.ascontiguousarray(v, F32), np.ascontiguousarray(f, np.int32), T.vertex_normals(v, f)


def _ring(n, H, W, radius=3.4):
    """n cameras around the test meshes, at varying heights, looking at their centre; float32 views [n, 16] and the poses."""
    K = R.intrinsics(H, W)
    poses = [R.look_at(S.CENTRE + radius * np.array([np.cos(2.4 * k + 0.3), 0.45 * np.sin(1.7 * k), np.sin(2.4 * k + 0.3)]), S.CENTRE)
             for k in range(n)]
    return np.stack([R.view_of(p, K) for p in poses]) if n else np.zeros((0, 16), F32), poses, K


def _gpu_maps(v, f, nrm, poses, K, H, W):
    """(depth, acc) [n, H W] numpy of the engine's rasteriser, which tests/test_gpu_raster.py holds to its reference: here they
    are inputs, the same for the kernel and for the reference."""
    from nerf_meets_mlx_amd.engine import mesh as E
    m = E.Mesh(_dev(v, torch.float32), _dev(f, torch.int32), _dev(nrm, torch.float32), None)
    both = [E.rasterize(m, p, K, H, W, NEAR)[2:4] for p in poses]
    return (np.stack([b[0].cpu().numpy().reshape(-1) for b in both]), np.stack([b[1].cpu().numpy().reshape(-1) for b in both]))


def _noise(n, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, H, W, 3, generator=g).numpy()


class Device:
    """A mesh, its views and their images and maps on the device, and the two C entries called as the engine calls them."""

    def __init__(self, v, f, nrm, texels, views, images, depth, acc):
        self.V, self.F, self.T = len(v), len(f), texels
        self.v, self.n, self.f = _dev(v, torch.float32), _dev(nrm, torch.float32), _dev(f, torch.int32)
        self.views = np.ascontiguousarray(views, F32)
        self.images, self.depth, self.acc = (_dev(a, torch.float32) for a in (images, depth, acc))
        self.H, self.W = images.shape[1:3]
        self.lay = T.layout(self.F, texels)
        self.P = self.lay[0] * self.lay[1]

    def state(self):
        """Zeroed, with a spare row that holds a pattern."""
        st = torch.zeros(self.P + 1, 4, dtype=torch.float32, device=DEV)
        st[self.P:].view(torch.uint8).fill_(POISON)
        return st

    def accumulate(self, st, mode, first=0, n=None, p0=0, count=None, tol=TOL, cos_min=COS_MIN, near=NEAR, acc_min=ACC_MIN):
        from nerf_meets_mlx_amd import _native as N
        n = len(self.views) - first if n is None else n
        count = self.P - p0 if count is None else count
        vw = np.ascontiguousarray(self.views[first:first + n])
        N.check(N.lib().nerf_project_accumulate(N.ptr(self.v), N.ptr(self.n), self.V, N.ptr(self.f), self.F, self.T, p0, count,
                                                vw.ctypes.data_as(C.POINTER(C.c_float)), n, self.H, self.W, N.ptr(self.images[first:first + n]),
                                                N.ptr(self.depth[first:first + n]), N.ptr(self.acc[first:first + n]), near, tol, cos_min,
                                                acc_min, mode, N.ptr(st), N.stream()))
        return st

    def batches(self, st, mode, size=P.MAX_VIEWS, **kw):
        for s in range(0, len(self.views), size):
            self.accumulate(st, mode, s, min(size, len(self.views) - s), **kw)
        return st

    def finish(self, st, mode, fallback=None, chunk=None):
        """(image [H, W, 3], seen [H, W]) uint8 numpy; the spare rows of both and of the state still hold their pattern."""
        from nerf_meets_mlx_amd import _native as N
        Wa, Ha = self.lay[:2]
        image = torch.full((Ha + 1, Wa, 3), POISON, dtype=torch.uint8, device=DEV)
        seen = torch.full((Ha + 1, Wa), POISON, dtype=torch.uint8, device=DEV)
        fb = None if fallback is None else _dev(fallback, torch.uint8)
        chunk = self.P if chunk is None else chunk
        for p0 in range(0, self.P, chunk):
            N.check(N.lib().nerf_project_finish(N.ptr(st), self.F, self.T, p0, min(chunk, self.P - p0), mode, N.ptr(fb), N.ptr(image),
                                                N.ptr(seen), N.stream()))
        assert bool((image[Ha:] == POISON).all()) and bool((seen[Ha:] == POISON).all())
        assert bool((st[self.P:].view(torch.uint8) == POISON).all())
        return image[:Ha].cpu().numpy(), seen[:Ha].cpu().numpy()

    def host_state(self, st):
        return st[:self.P].cpu().numpy()


def _same(got, want, what):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    bad = np.nonzero(got != want)[0]
    assert got.shape == want.shape and len(bad) == 0, (what, len(bad), bad[:4], got[bad[:4]], want[bad[:4]])


def _reference(v, f, nrm, texels, views, images, depth, acc, mode, fallback=None, tol=TOL, cos_min=COS_MIN, near=NEAR):
    lay = T.layout(len(f), texels)
    state = np.zeros((lay[0] * lay[1], 4), F32)
    P.accumulate(state, v, nrm, f, texels, views, images, depth, acc, near, tol, cos_min, ACC_MIN, mode)
    return (state,) + P.finish(state, lay, mode, fallback)


def _check(d, v, f, nrm, images, depth, acc, mode, fallback=None, what="", **kw):
    """The device's state, image and seen of all views, in launches of at most 16, against the reference's, as integers."""
    st = d.batches(d.state(), mode, **kw)
    image, seen = d.finish(st, mode, fallback)
    want = _reference(v, f, nrm, d.T, d.views, images, depth, acc, mode, fallback, **kw)
    _same(d.host_state(st).view(np.int32), want[0].view(np.int32), what + " state")
    _same(image, want[1], what + " image")
    _same(seen, want[2], what + " seen")
    return want


# ------------------------------------------------------------------------------------------------ bit-identity
CASES = [(list(MESHES)[i % 4], (2, 3, 8)[i % 3], n, mode, hw)
         for i, (n, mode, hw) in enumerate(itertools.product((1, 2, 16, 17), (P.BLEND, P.BEST), ((17, 33), (96, 96))))]


@pytest.mark.parametrize("name,texels,n,mode,hw", CASES)
def test_state_image_and_seen_equal_the_reference(name, texels, n, mode, hw):
    """Every mesh, T, image size, mode and number of views at least once (the meshes and T cycle with coprime periods over the
    16 combinations of n, mode and size); 17 views make a second launch."""
    H, W = hw
    v, f, nrm = _mesh(name)
    views, poses, K = _ring(n, H, W)
    depth, acc = _gpu_maps(v, f, nrm, poses, K, H, W)
    images = _noise(n, H, W, seed=n + 100 * texels)
    d = Device(v, f, nrm, texels, views, images, depth, acc)
    fallback = np.random.default_rng(n).integers(0, 256, (d.lay[1], d.lay[0], 3)).astype(np.uint8)
    state, image, seen = _check(d, v, f, nrm, images, depth, acc, mode, fallback if n % 2 else None, what=f"{name} T={texels} n={n}")
    ok = P.texels(v, nrm, f, texels)[0]
    print(name, "T", texels, "n", n, "mode", mode, hw, "texels", d.P, "of faces", int(ok.sum()), "seen", int(seen.sum()))
    if name.startswith("sphere"):                                          # (the reference sees 24 % of sphere12 with one view)
        assert seen.sum() > 0.1 * ok.sum()
    assert not seen.reshape(-1)[~ok].any()


# ------------------------------------------------------------------------------------------------ invariance
@pytest.fixture(scope="module")
def scene():
    """sphere12 at T = 3 under 16 views of 17 x 33 noise, and its reference, computed once."""
    v, f, nrm = _mesh("sphere12")
    H, W = 17, 33
    views, poses, K = _ring(16, H, W)
    depth, acc = _gpu_maps(v, f, nrm, poses, K, H, W)
    images = _noise(16, H, W, seed=5)
    d = Device(v, f, nrm, 3, views, images, depth, acc)
    want = {mode: _reference(v, f, nrm, 3, views, images, depth, acc, mode) for mode in (P.BLEND, P.BEST)}
    return d, want


@pytest.mark.parametrize("mode", [P.BLEND, P.BEST])
def test_chunks_repeats_and_the_split_of_the_views_change_no_bit(scene, mode):
    d, want = scene
    Wa = d.lay[0]
    state, image, seen = want[mode]
    assert seen.sum() > 1000
    for chunk in (Wa + 1, d.P):
        for rep in range(2):
            st = d.state()
            for p0 in range(0, d.P, chunk):
                d.accumulate(st, mode, p0=p0, count=min(chunk, d.P - p0))
            _same(d.host_state(st).view(np.int32), state.view(np.int32), f"chunk {chunk} run {rep}")
            got = d.finish(st, mode, chunk=chunk)
            _same(got[0], image, f"chunk {chunk} image")
            _same(got[1], seen, f"chunk {chunk} seen")
    # one launch of 16 views, 16 launches of one, and launches of 5
    for size in (1, 5):
        _same(d.host_state(d.batches(d.state(), mode, size=size)).view(np.int32), state.view(np.int32), f"launches of {size} views")


@pytest.mark.parametrize("chunk", [1, 7])
def test_the_smallest_chunks(chunk):
    """The tetrahedron at T = 2: an atlas of 32 texels, cut into chunks of 1 and of 7 for both entries.  Its texels sit on the
    vertices, on the silhouette of most views: 96 x 96 pixels and a wide depth_tol for a handful of observations."""
    v, f, nrm = _mesh("tetrahedron")
    H, W = 96, 96
    views, poses, K = _ring(2, H, W)
    depth, acc = _gpu_maps(v, f, nrm, poses, K, H, W)
    images = _noise(2, H, W, seed=9)
    d = Device(v, f, nrm, 2, views, images, depth, acc)
    assert d.P == 32
    for mode in (P.BLEND, P.BEST):
        state, image, seen = _reference(v, f, nrm, 2, views, images, depth, acc, mode, tol=0.5)
        st = d.state()
        for p0 in range(0, d.P, chunk):
            d.accumulate(st, mode, p0=p0, count=min(chunk, d.P - p0), tol=0.5)
        _same(d.host_state(st).view(np.int32), state.view(np.int32), "state")
        got = d.finish(st, mode, chunk=chunk)
        _same(got[0], image, "image")
        _same(got[1], seen, "seen")
        assert seen.sum() >= 4


# ------------------------------------------------------------------------------------------------ edge cases
def test_nan_in_the_maps_and_the_images_drops_the_observation():
    v, f, nrm = _mesh("sphere12")
    H, W = 17, 33
    views, poses, K = _ring(3, H, W)
    depth, acc = _gpu_maps(v, f, nrm, poses, K, H, W)
    images = _noise(3, H, W, seed=21)
    clean = _reference(v, f, nrm, 8, views, images, depth, acc, P.BLEND)[2]
    rng = np.random.default_rng(22)
    depth, acc, images = depth.copy(), acc.copy(), images.copy()
    depth[rng.random(depth.shape) < 0.1] = np.nan
    acc[rng.random(acc.shape) < 0.1] = np.nan
    images[rng.random(images.shape) < 0.03] = np.nan
    images[rng.random(images.shape) < 0.01] = np.inf
    depth[0, :5], acc[1, :5] = -np.inf, np.inf
    d = Device(v, f, nrm, 8, views, images, depth, acc)
    for mode in (P.BLEND, P.BEST):
        state, image, seen = _check(d, v, f, nrm, images, depth, acc, mode, what="NaN")
        assert 0 < seen.sum() < clean.sum()
        got = state[seen.reshape(-1) == 1]
        assert not np.isnan(got).any()                                     # no NaN observation entered a texel that counts as seen


def test_bad_faces_make_no_observation():
    v, f, nrm = _mesh("sphere12")
    V = len(v)
    f = f.copy()
    big = np.iinfo(np.int32)
    a, b = int(f[0, 0]), int(f[0, 1])
    f[1], f[4], f[9], f[14], f[len(f) - 1] = [a, b, V], [-1, a, b], [a, big.max, b], [a, b, big.min], [V, V, V]
    H, W = 17, 33
    views, poses, K = _ring(2, H, W)
    depth, acc = _gpu_maps(v, f, nrm, poses, K, H, W)
    images = _noise(2, H, W, seed=31)
    d = Device(v, f, nrm, 3, views, images, depth, acc)
    fallback = np.full((d.lay[1], d.lay[0], 3), 9, np.uint8)
    ok = P.texels(v, nrm, f, 3)[0]
    p = np.arange(d.P)
    face = T.owner(d.lay, p % d.lay[0], p // d.lay[0])[0]
    assert not ok[np.isin(face, [1, 4, 9, 14, len(f) - 1])].any()
    for mode in (P.BLEND, P.BEST):
        state, image, seen = _check(d, v, f, nrm, images, depth, acc, mode, fallback, what="bad faces")
        assert not seen.reshape(-1)[~ok].any() and (image.reshape(-1, 3)[~ok] == 9).all() and not state[~ok].any()
        assert seen.sum() > 500


def test_texels_outside_the_image_and_behind_the_near_plane():
    """A camera inside the sphere: much of the mesh is behind it or in front of `near`, much projects outside the image."""
    v, f, nrm = _mesh("sphere12")
    H, W = 17, 33
    K = R.intrinsics(H, W)
    poses = [R.look_at(S.CENTRE + [0.2, 0.1, 0.3], S.CENTRE + [2.0, 0.3, 0.1]), R.look_at(S.CENTRE + [-1.2, 0.4, 2.0], S.CENTRE + [0.9, 0.5, 0.0])]
    views = np.stack([R.view_of(p, K) for p in poses])
    near = 0.6
    nrm_in = -nrm                                                           # seen from inside, the inner side faces the camera
    images = _noise(2, H, W, seed=41)
    ok, x, _ = P.texels(v, nrm_in, f, 8)
    u, w, zc = R.project(x, views[0])
    assert (ok & (zc < 0)).sum() > 1000 and (ok & (zc > 0) & (zc < near)).sum() > 100 and (ok & (zc > near) & ((u < 0) | (u > W))).sum() > 100
    for normals in (nrm_in, nrm):
        depth, acc = _gpu_maps(v, f, normals, poses, K, H, W)
        d = Device(v, f, normals, 8, views, images, depth, acc)
        for mode in (P.BLEND, P.BEST):
            seen = _check(d, v, f, normals, images, depth, acc, mode, what="inside", near=near)[2]
            assert seen.any()


@pytest.mark.parametrize("hw", [(2, 2), (1, 7), (7, 1), (2, 9)])
def test_the_smallest_images(hw):
    """2 x 2 is the smallest image with room for a bilinear footprint; one that is a single pixel high or wide has none, and
    nothing is seen."""
    H, W = hw
    v, f, nrm = _mesh("sphere12")
    views, poses, K = _ring(3, H, W, radius=12.0)
    depth, acc = _gpu_maps(v, f, nrm, poses, K, H, W)
    images = _noise(3, H, W, seed=51)
    d = Device(v, f, nrm, 8, views, images, depth, acc)
    for mode in (P.BLEND, P.BEST):
        seen = _check(d, v, f, nrm, images, depth, acc, mode, what=f"{H} x {W}")[2]
        assert bool(seen.any()) == (min(H, W) >= 2)


def test_no_faces_and_no_views_on_the_device():
    from nerf_meets_mlx_amd.engine import mesh as E
    v, f, nrm = _mesh("sphere12")
    H, W = 6, 8
    views, poses, K = _ring(2, H, W)
    images = _dev(_noise(2, H, W, seed=61), torch.float32)
    dv, dn = _dev(v, torch.float32), _dev(nrm, torch.float32)
    empty = E.Mesh(dv, torch.zeros(0, 3, dtype=torch.int32, device=DEV), dn)
    tex, seen = E.project_texture(empty, images, np.stack(poses), K, 6, TOL)
    assert tex.image.shape == (8, 8, 3) and not tex.image.any() and not seen.any() and tex.uv.shape == (0, 3, 2)
    m = E.Mesh(dv, _dev(f, torch.int32), dn)
    fb = E.Texture(torch.full((T.layout(len(f), 2)[1], T.layout(len(f), 2)[0], 3), 7, dtype=torch.uint8, device=DEV),
                   torch.zeros(len(f), 3, 2, device=DEV), 2)
    for fallback, byte in ((fb, 7), (None, 0)):
        tex, seen = E.project_texture(m, images[:0], np.zeros((0, 3, 4)), K, 2, TOL, fallback=fallback)
        assert bool((tex.image == byte).all()) and not seen.any()
        assert np.array_equal(tex.uv.cpu().numpy().view(np.int32), T.uvs(len(f), 2).view(np.int32))


# ------------------------------------------------------------------------------------------------ end to end
def test_constant_images_through_the_engine_with_its_own_maps(tmp_path):
    """Property 1 of tests/test_project_host.py through engine.mesh.project_texture, which rasterises the views itself: equal to the
    reference with the reference rasteriser's maps; and what it returns goes through render_mesh and write_obj."""
    from nerf_meets_mlx_amd.engine import mesh as E
    v, f = S.sphere(24)
    nrm = T.vertex_normals(v, f)
    H = W = 96
    K = R.intrinsics(H, W)
    poses = [R.look_at(S.CENTRE + [2.6, 1.1, 2.2], S.CENTRE), R.look_at(S.CENTRE + [-2.0, -0.7, 2.4], S.CENTRE)]
    views = np.stack([R.view_of(p, K) for p in poses])
    images = np.zeros((2, H, W, 3), F32)
    images[0, ..., 0], images[1, ..., 1] = 1.0, 1.0
    m = E.Mesh(_dev(v, torch.float32), _dev(f, torch.int32), _dev(nrm, torch.float32), None)
    lay = T.layout(len(f), 8)
    fb_bytes = np.random.default_rng(3).integers(0, 256, (lay[1], lay[0], 3)).astype(np.uint8)
    fb = E.Texture(_dev(fb_bytes, torch.uint8), _dev(T.uvs(len(f), 8), torch.float32), 8)
    ok, x, n = P.texels(v, nrm, f, 8)
    maps = [P.maps(v, f, vw, H, W, NEAR) for vw in views]
    a, b = (P.observe(views[k], images[k], maps[k][0], maps[k][1], x, n, NEAR, TOL, COS_MIN, ACC_MIN)[0] & ok for k in range(2))
    assert (a & ~b).sum() > 500 and (b & ~a).sum() > 500 and (a & b).sum() > 200
    for mode in ("blend", "best"):
        tex, seen = E.project_texture(m, _dev(images, torch.float32), np.stack(poses), K, 8, TOL, mode=mode, fallback=fb, chunk=50001,
                                          cos_min=COS_MIN)
        want = P.bake(v, nrm, f, 8, views, images, NEAR, TOL, COS_MIN, ACC_MIN, P.MODES[mode], fb_bytes,
                      np.stack([mp[0] for mp in maps]), np.stack([mp[1] for mp in maps]))
        _same(tex.image.cpu().numpy(), want[0], mode + " image")
        _same(seen.cpu().numpy(), want[1], mode + " seen")
        _same(tex.uv.cpu().numpy().view(np.int32), T.uvs(len(f), 8).view(np.int32), "uv")
        px = tex.image.cpu().numpy().reshape(-1, 3).astype(np.int64)
        assert (px[a & ~b] == [255, 0, 0]).all() and (px[b & ~a] == [0, 255, 0]).all()
        assert np.array_equal(px[~a & ~b], fb_bytes.reshape(-1, 3)[~a & ~b])
        both = px[a & b]
        if mode == "blend":
            assert (both[:, 2] == 0).all() and (np.abs(both[:, 0] + both[:, 1] - 255) <= 1).all()
        else:
            assert (((both == [255, 0, 0]).all(1)) | ((both == [0, 255, 0]).all(1))).all()
    # the maps handed over are the maps it would have made
    d, ac = (_dev(np.stack([mp[k] for mp in maps]).reshape(2, H, W), torch.float32) for k in (0, 1))
    again, seen2 = E.project_texture(m, _dev(images, torch.float32), np.stack(poses), K, 8, TOL, mode="best", fallback=fb, depth=d, acc=ac,
                                     cos_min=COS_MIN)
    assert torch.equal(again.image, tex.image) and torch.equal(seen2, seen)
    # the renderer and the writer take the result: with best, most of what view 0 sees took view 0's red
    frame = E.render_mesh(m, poses[0], K, H, W, texture=tex)
    rgb = frame.rgb.cpu().numpy()
    hit = frame.face.cpu().numpy() >= 0
    red = (rgb[hit][:, 0] > 0.99) & (rgb[hit][:, 1:] < 0.01).all(1)          # (the others touch a texel only the fallback colours)
    print("render through the projected texture: red", int(red.sum()), "of", int(hit.sum()), "covered pixels")
    assert hit.sum() > 1000 and red.sum() > 0.4 * hit.sum()     # (view 1, 100 degrees away, wins about a third of the disc)
    path = E.write_obj(str(tmp_path / "projected.obj"), E.Mesh(m.verts.cpu(), m.faces.cpu(), m.normals.cpu(), None),
                       E.Texture(tex.image.cpu(), tex.uv.cpu(), tex.texels))
    back = E.read_obj(path)[1]
    assert torch.equal(back.image, tex.image.cpu()) and back.texels == 8


def test_seventeen_views_through_the_engine():
    """The engine cuts 17 views into launches of 16 and 1 and rasterises each: equal to the reference fed the same maps."""
    from nerf_meets_mlx_amd.engine import mesh as E
    v, f, nrm = _mesh("sphere12")
    H, W = 17, 33
    views, poses, K = _ring(17, H, W)
    depth, acc = _gpu_maps(v, f, nrm, poses, K, H, W)
    images = _noise(17, H, W, seed=71)
    m = E.Mesh(_dev(v, torch.float32), _dev(f, torch.int32), _dev(nrm, torch.float32), None)
    for mode in ("blend", "best"):
        tex, seen = E.project_texture(m, _dev(images, torch.float32), np.stack(poses), K, 3, TOL, mode=mode, chunk=999, cos_min=COS_MIN)
        want = _reference(v, f, nrm, 3, views, images, depth, acc, P.MODES[mode])
        _same(tex.image.cpu().numpy(), want[1], mode + " image")
        _same(seen.cpu().numpy(), want[2], mode + " seen")


def test_trainer_project_texture_of_constant_training_images():
    """A tiny untrained trainer whose training images are one colour, (0.25, 0.5, 0.75): every texel a camera sees takes that
    colour, every other texel texture_mesh's.  The seen bytes are (64, 128, 191) up to the rule's own rounding: 0.5 * 255 = 127.5
    lies on a rounding boundary, and the bilinear weights of a texel sum to 1 - 2^-24 for some texels, so the green byte of
    those is 127 (the numpy reference on sphere12 at T = 4 and 8 x 8 images: 80 of 4694 seen texels).  Red and blue are exact;
    green is held to 128 or 127, within the half byte step of the affine property, and at least nine in ten are 128."""
    from nerf_meets_mlx_amd.dataset import synthetic
    from nerf_meets_mlx_amd.engine import mesh as E
    from nerf_meets_mlx_amd.engine.trainer import Trainer
    imgs, poses, _, _, K = synthetic.make_dataset(8, 8, 3, seed=0, device=DEV)
    imgs = torch.tensor([0.25, 0.5, 0.75], device=DEV).expand(3, 8, 8, 3).contiguous()
    tr = Trainer(imgs, poses, K, N_rand=64, n_depth_samples=16, N_importance=16, seed=4, device=DEV)
    box = ([-1.0] * 3, [1.0] * 3)
    vol = tr.density_volume(16, box)
    m = tr.extract_mesh(resolution=16, threshold=float(vol.reshape(-1).quantile(0.7)), aabb=box)
    assert m.faces.shape[0] > 0
    base = tr.texture_mesh(m, 4)
    for mode in ("blend", "best"):
        tex, seen = tr.project_texture(m, texels=4, mode=mode, depth_tol=0.3)
        got = seen.bool().reshape(-1)
        px = tex.image.reshape(-1, 3)
        print("trainer", mode, "seen", int(got.sum()), "of", got.numel(), "green 127:", int((px[got][:, 1] == 127).sum()))
        assert got.sum() > 50 and (~got).sum() > 50
        assert bool((px[got][:, 0] == 64).all()) and bool((px[got][:, 2] == 191).all())
        assert bool(((px[got][:, 1] == 128) | (px[got][:, 1] == 127)).all()) and (px[got][:, 1] == 128).float().mean() > 0.9
        assert torch.equal(px[~got], base.image.reshape(-1, 3)[~got]) and torch.equal(tex.uv, base.uv)
    # a subset of the views, the field's own pictures (drawn with the trainer's random stream), no fallback
    tex, seen1 = tr.project_texture(m, texels=4, views=[1], source="field", fallback=False, depth_tol=0.3)
    want = E.project_texture(m, imgs[1:2].contiguous(), tr.poses[1:2, :3, :4], tr.K, 4, 0.3, near=float(tr.near))
    assert torch.equal(seen1, want[1]) and 0 < int(seen1.sum()) < int(seen.sum())
    assert not bool(tex.image.reshape(-1, 3)[~seen1.bool().reshape(-1)].any()) and bool(tex.image.any())
    with pytest.raises(ValueError, match="pass depth_tol"):
        tr.project_texture(m, texels=4)
    with pytest.raises(ValueError, match="views"):
        tr.project_texture(m, texels=4, views=[3], depth_tol=0.3)
