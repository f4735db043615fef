"""The texture mip pyramid on the GPU (csrc/mip.hip, engine/mesh build_mipmaps / face_lod / sample_texture_mip / render_mesh_mip,
Trainer.mip_texture / render_mesh_mip / mesh_psnr_mip) against the numpy reference of tests/_mip_ref.py: bytes and float bits
compared as integers -- no tolerance, the rule is exact -- into poisoned or sentinel-filled outputs."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import _mip_ref as M
from tests import _raster_ref as R
from tests import _smooth_ref as S
from tests import _texture_ref as T
from tests._poison import bits_equal, sentinel_, unwritten

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL = 0xA5                                                            # what a coarse image holds before a reduce
NEAR = 0.01
POSES = [R.look_at(S.CENTRE + [2.6, 1.1, 2.2], S.CENTRE), R.look_at(S.CENTRE + [-1.2, 0.4, 2.0], S.CENTRE + [0.9, 0.5, 0.0])]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"


def _dev(a, dtype):
    return torch.from_numpy(np.array(a, order="C")).to(device=DEV, dtype=dtype).contiguous()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _soup(F=37):
    rng = np.random.default_rng(37)
    v = (rng.standard_normal((40, 3)) * [1.0, 0.8, 1.2] + S.CENTRE).astype(np.float32)
    f = np.stack([rng.permutation(40)[:3] for _ in range(37)]).astype(np.int32)
    return v, f[:F]


MESHES = {"tetrahedron": S.tetrahedron, "one": lambda: _soup(1), "five": lambda: _soup(5), "soup37": _soup,
          "sphere12": lambda: S.sphere(12), "sphere24": lambda: S.sphere(24)}


@functools.lru_cache(maxsize=None)
def _mesh_np(name):
    v, f = MESHES[name]()
    v, f = np.asarray(v, np.float32), np.asarray(f, np.int32)
    return v, f, T.vertex_normals(v, f)


def _mesh(name):
    from nerf_meets_mlx_amd.engine import mesh as E
    v, f, n = _mesh_np(name)
    return E.Mesh(_dev(v, torch.float32), _dev(f, torch.int32), _dev(n, torch.float32), None)


@functools.lru_cache(maxsize=None)
def _random_atlas(F, texels):
    """Random bytes in every texel, the unused ones included: the reduce must not look at them."""
    W, H = T.layout(F, texels)[:2]
    img = np.random.default_rng(1000 * F + texels).integers(0, 256, (H, W, 3)).astype(np.uint8)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _ref_pyramid(F, texels):
    """The reference pyramid over the random atlas, computed once and shared: [(image, uv, T_l)]."""
    out = M.pyramid(_random_atlas(F, texels), F, texels)
    for im, uv, _ in out:
        im.setflags(write=False)
        uv.setflags(write=False)
    return out


def _texture(F, texels):
    from nerf_meets_mlx_amd.engine import mesh as E
    return E.Texture(_dev(_random_atlas(F, texels), torch.uint8), _dev(T.uvs(F, texels), torch.float32), texels)


def _c_reduce(fine, F, texels, chunk):
    """nerf_mip_reduce chunk by chunk into an image that holds FILL, with four spare bytes behind it."""
    from nerf_meets_mlx_amd import _native as N
    W, H = T.layout(F, (texels + 1) // 2)[:2]
    image = torch.full((H * W * 3 + 4,), FILL, dtype=torch.uint8, device=DEV)
    for p0 in range(0, W * H, chunk):
        N.check(N.lib().nerf_mip_reduce(N.ptr(fine), F, texels, N.ptr(image), p0, min(chunk, W * H - p0), N.stream()))
    assert bool((image[H * W * 3:] == FILL).all())                     # nothing is written behind the image
    return image[:H * W * 3].view(H, W, 3)


# ------------------------------------------------------------------------------------------------ reduce
@pytest.mark.parametrize("texels", [3, 4, 8, 9])
@pytest.mark.parametrize("name,F", [("tetrahedron", 4), ("one", 1), ("five", 5), ("soup37", 37), ("sphere12", 768)])
def test_reduce_matches_the_reference_bit_for_bit_whatever_the_chunk(name, F, texels):
    assert len(_mesh_np(name)[1]) == F
    fine = _dev(_random_atlas(F, texels), torch.uint8)
    want = _ref_pyramid(F, texels)[1][0]
    W, H = T.layout(F, (texels + 1) // 2)[:2]
    assert want.shape == (H, W, 3)
    whole = _c_reduce(fine, F, texels, W * H)
    got = whole.cpu().numpy()
    assert np.array_equal(got, want), ("bytes differ", np.argwhere((got != want).any(2))[:4])
    lc = T.layout(F, (texels + 1) // 2)
    Y, X = np.mgrid[0:H, 0:W]
    unused = T.owner(lc, X, Y)[0] >= F
    assert not got[unused].any() and got[~unused].any()
    for chunk in (1, 7):
        assert torch.equal(_c_reduce(fine, F, texels, chunk), whole), chunk
    assert torch.equal(_c_reduce(fine, F, texels, W * H), whole)       # two runs agree
    # a chunk that starts and ends inside a workgroup's span touches nothing else
    from nerf_meets_mlx_amd import _native as N
    p0 = min(W * H - 1, 259)
    cnt = min(W * H - p0, 300)
    part = torch.full((H * W, 3), FILL, dtype=torch.uint8, device=DEV)
    N.check(N.lib().nerf_mip_reduce(N.ptr(fine), F, texels, N.ptr(part), p0, cnt, N.stream()))
    part = part.cpu().numpy()
    assert np.array_equal(part[p0:p0 + cnt], want.reshape(-1, 3)[p0:p0 + cnt])
    assert (part[:p0] == FILL).all() and (part[p0 + cnt:] == FILL).all()


# ------------------------------------------------------------------------------------------------ level of detail
def _lod_scene():
    """sphere24 and four faces the rasteriser drops: a degenerate one, one with a vertex between the camera and `near` for each of
    the two poses, and one with an index outside [0, V)."""
    v, f, _ = _mesh_np("sphere24")
    V = len(v)
    extra = np.array([R.from_camera(c, 0.0, 0.001, 0.5 * NEAR) for c in POSES], np.float32)
    a, b = int(f[0, 0]), int(f[0, 1])
    bad = np.array([[a, a, b], [a, b, V], [V + 1, a, b], [a, b, V + 2]], np.int32)
    return np.concatenate([v, extra]), np.concatenate([f, bad]), len(f)


@pytest.mark.parametrize("texels", [2, 8, 9])
@pytest.mark.parametrize("hw", [(48, 64), (96, 96)])
@pytest.mark.parametrize("pose", [0, 1])
def test_face_lod_matches_the_reference_bit_for_bit(pose, hw, texels):
    from nerf_meets_mlx_amd import _native as N
    from nerf_meets_mlx_amd.engine import mesh as E
    v, f, F0 = _lod_scene()
    mesh = E.Mesh(_dev(v, torch.float32), _dev(f, torch.int32), torch.zeros(len(v), 3, device=DEV), None)
    K = R.intrinsics(*hw)
    view = R.view_of(POSES[pose], K)
    L = len(M.levels(texels))
    for scale in (0.5, 1.0, 2.0):
        want = M.face_lod(v, f, view, NEAR, texels, scale)
        got = E.face_lod(mesh, POSES[pose], K, near=NEAR, texels=texels, scale=scale)
        assert got.shape == (len(f),) and np.array_equal(_bits(got.cpu().numpy()), _bits(want)), (scale, np.nonzero(_bits(got.cpu().numpy()) != _bits(want))[0][:4])
        assert not want[[F0, F0 + 1 + pose, F0 + 3]].any()               # degenerate, behind near, index outside [0, V)
        assert want.min() >= 0.0 and want.max() <= L - 1
        if texels == 2:
            assert not want.any()
    if texels != 2:
        want = M.face_lod(v, f, view, NEAR, texels, 1.0)
        assert (want != np.floor(want)).any() and len(np.unique(np.floor(want))) >= 2
    # through the C entry into a sentinel-filled buffer: F elements written and no more
    out = sentinel_(torch.empty(len(f) + 1, dtype=torch.float32, device=DEV))
    vp = np.ascontiguousarray(view, np.float32).ctypes.data_as(C.POINTER(C.c_float))
    N.check(N.lib().nerf_mip_lod(N.ptr(mesh.verts), len(v), N.ptr(mesh.faces), len(f), vp, NEAR, texels, 1.0, N.ptr(out), N.stream()))
    assert unwritten(out[len(f):]) == 1 and unwritten(out[:len(f)]) == 0


# ------------------------------------------------------------------------------------------------ lookup
def _samples(F, L, n=1500, seed=0):
    rng = np.random.default_rng(seed + F)
    sf = rng.integers(0, F, n).astype(np.int32)
    sf[:8] = [-1, F, F + 1, -2 ** 31, 2 ** 31 - 1, 0, F - 1, F - 1]
    sb = rng.dirichlet([1, 1, 1], n)[:, 1:].astype(np.float32)
    sb[8:20] = [[0, 0], [1, 0], [0, 1], [0.5, 0.5], [0.5, 0], [0, 0.5], [-0.5, 0.5], [0.7, 0.7], [np.nan, 0.5], [0.5, np.nan], [2, 2], [1, 1]]
    lod = rng.uniform(0.0, max(L - 1, 1), n).astype(np.float32)
    return sf, sb, lod


@pytest.mark.parametrize("name,texels", [("soup37", 9), ("five", 8), ("sphere12", 8), ("tetrahedron", 2), ("one", 3)])
def test_trilinear_lookup(name, texels):
    from nerf_meets_mlx_amd import _native as N
    from nerf_meets_mlx_amd.engine import mesh as E
    mesh = _mesh(name)
    F = mesh.faces.shape[0]
    ref = _ref_pyramid(F, texels)
    L = len(ref)
    pyr = E.TexturePyramid(tuple(E.Texture(_dev(im, torch.uint8), _dev(uv, torch.float32), tl) for im, uv, tl in ref))
    images = [im for im, _, _ in ref]
    sf, sb, lod = _samples(F, L)
    tf, tb = _dev(sf, torch.int32), _dev(sb, torch.float32)
    n = len(sf)
    # an integral lod is sample_texture on that level
    for l in range(L):
        got = E.sample_texture_mip(pyr, mesh, tf, tb, torch.full((n,), float(l), device=DEV))
        assert bits_equal(got, E.sample_texture(pyr.levels[l], mesh, tf, tb)), l
    # fractional: against the reference, into a sentinel-filled buffer
    want = M.sample(images, F, texels, sf, sb, lod)
    out = sentinel_(torch.empty(n + 1, 3, dtype=torch.float32, device=DEV))
    ptrs = (C.c_void_p * L)(*[t.image.data_ptr() for t in pyr.levels])
    N.check(N.lib().nerf_mip_sample(ptrs, F, texels, N.ptr(tf), N.ptr(tb), N.ptr(_dev(lod, torch.float32)), 0, n, N.ptr(out), N.stream()))
    assert unwritten(out[n:]) == 3 and unwritten(out[:n]) == 0
    assert np.array_equal(_bits(out[:n].cpu().numpy()), _bits(want))
    assert bits_equal(E.sample_texture_mip(pyr, mesh, tf, tb, _dev(lod, torch.float32)), out[:n])
    assert not want[:5].any() and want.any()                             # faces outside [0, F) read black
    # per face: the lod gathered at the sample's face
    flod = np.random.default_rng(texels).uniform(-0.5, L - 0.5, F).astype(np.float32)
    gathered = flod[np.clip(sf.astype(np.int64), 0, F - 1)]
    got = E.sample_texture_mip(pyr, mesh, tf, tb, _dev(flod, torch.float32), per_face=True)
    assert bits_equal(got, E.sample_texture_mip(pyr, mesh, tf, tb, _dev(gathered, torch.float32)))
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(M.sample(images, F, texels, sf, sb, flod, per_face=True)))
    # NaN, -1 and 99 read level 0, level 0 and level L - 1
    for value, level in ((float("nan"), 0), (-1.0, 0), (99.0, L - 1), (float("inf"), L - 1), (float("-inf"), 0)):
        got = E.sample_texture_mip(pyr, mesh, tf, tb, torch.full((n,), value, device=DEV))
        assert bits_equal(got, E.sample_texture(pyr.levels[level], mesh, tf, tb)), value


# ------------------------------------------------------------------------------------------------ build_mipmaps
@pytest.mark.parametrize("name,texels", [("soup37", 9), ("five", 8), ("sphere12", 4), ("tetrahedron", 2)])
def test_build_mipmaps_gives_the_reference_pyramid(name, texels):
    from nerf_meets_mlx_amd.engine import mesh as E
    mesh = _mesh(name)
    F = mesh.faces.shape[0]
    tex = _texture(F, texels)
    ref = _ref_pyramid(F, texels)
    stages = []
    pyr = E.build_mipmaps(tex, mesh, mark=stages.append)
    assert isinstance(pyr, E.TexturePyramid) and pyr.levels[0] is tex and len(pyr.levels) == len(ref)
    assert stages == ["reduce", "uv"] * (len(ref) - 1)
    assert tuple(t.texels for t in pyr.levels) == E.mip_levels(texels) == M.levels(texels)
    for level, (im, uv, tl) in zip(pyr.levels, ref):
        assert level.texels == tl and np.array_equal(level.image.cpu().numpy(), im), tl
        assert np.array_equal(_bits(level.uv.cpu().numpy()), _bits(uv)), tl
        E._check_texture("test", level, mesh)                            # every level is a complete Texture of the mesh
    for chunk in (1 if F < 100 else 1001, 7 if F < 100 else 4099):
        other = E.build_mipmaps(tex, mesh, chunk=chunk)
        assert all(torch.equal(a.image, b.image) and bits_equal(a.uv, b.uv) for a, b in zip(other.levels, pyr.levels)), chunk
    with pytest.raises(ValueError):
        E.sample_texture_mip(E.TexturePyramid(pyr.levels + pyr.levels[-1:]), mesh, torch.zeros(0, dtype=torch.int32, device=DEV),
                             torch.zeros(0, 2, device=DEV), torch.zeros(0, device=DEV))


# ------------------------------------------------------------------------------------------------ render
@pytest.mark.parametrize("per_pixel", [False, True])
def test_render_mesh_mip_is_the_reference_composition(per_pixel):
    from nerf_meets_mlx_amd.engine import mesh as E
    H, W, texels = 48, 64, 8
    v, f, _ = _mesh_np("sphere24")
    mesh = _mesh("sphere24")
    F = len(f)
    tex = _texture(F, texels)
    pyr = E.build_mipmaps(tex, mesh)
    ref = _ref_pyramid(F, texels)
    assert all(np.array_equal(a.image.cpu().numpy(), b[0]) for a, b in zip(pyr.levels, ref))
    K = R.intrinsics(H, W)
    rng = np.random.default_rng(5)
    bg = rng.uniform(0, 1, (H * W, 3)).astype(np.float32) if per_pixel else np.array([0.125, 0.5, 0.875], np.float32)
    stages = []
    fr = E.render_mesh_mip(mesh, POSES[0], K, H, W, pyr, background=_dev(bg, torch.float32), near=NEAR, mark=stages.append)
    assert stages == ["clear", "draw", "resolve", "lod", "texture", "shade"]
    rgb, face, bary, depth, acc, lod = M.render(v, f, R.view_of(POSES[0], K), H, W, NEAR, [im for im, _, _ in ref], texels, bg)
    hit = face >= 0
    assert 300 < hit.sum() < H * W - 300 and (lod[face[hit]] > 0).any() and len(np.unique(np.floor(lod[face[hit]]))) >= 2
    assert np.array_equal(_bits(fr.rgb.cpu().numpy().reshape(-1, 3)), _bits(rgb))
    plain = E.render_mesh(mesh, POSES[0], K, H, W, texture=tex, background=_dev(bg, torch.float32), near=NEAR)
    for name in ("face", "bary", "depth", "acc"):
        assert bits_equal(getattr(fr, name), getattr(plain, name)), name
    assert np.array_equal(fr.face.cpu().numpy().reshape(-1), face)
    assert not bits_equal(fr.rgb, plain.rgb)
    sharp = E.render_mesh_mip(mesh, POSES[0], K, H, W, pyr, background=_dev(bg, torch.float32), near=NEAR, lod_scale=1e6)
    assert not E.face_lod(mesh, POSES[0], K, NEAR, texels, 1e6).any() and bits_equal(sharp.rgb, plain.rgb)


# ------------------------------------------------------------------------------------------------ trainer, empty mesh
def test_trainer_mip_texture_render_mesh_mip_and_mesh_psnr_mip():
    from nerf_meets_mlx_amd.dataset import synthetic
    from nerf_meets_mlx_amd.engine import mesh as E
    from nerf_meets_mlx_amd.engine.trainer import Trainer
    imgs, poses, _, _, K = synthetic.make_dataset(8, 8, 2, seed=0, device=DEV)
    tr = Trainer(imgs, poses, K, N_rand=64, n_depth_samples=16, N_importance=16, seed=4, device=DEV)
    box = ([-1.0] * 3, [1.0] * 3)
    vol = tr.density_volume(16, box)
    m = tr.extract_mesh(resolution=16, threshold=float(vol.reshape(-1).quantile(0.7)), aabb=box)
    assert m.faces.shape[0] > 0
    c2w = poses[0].cpu().numpy() if torch.is_tensor(poses) else np.asarray(poses[0])
    tex = tr.texture_mesh(m, texels=8)
    pyr = tr.mip_texture(m, tex)
    want = E.build_mipmaps(tex, m)
    assert pyr.levels[0] is tex and tuple(t.texels for t in pyr.levels) == (8, 4, 2)
    assert all(torch.equal(a.image, b.image) and bits_equal(a.uv, b.uv) for a, b in zip(pyr.levels, want.levels))
    host = M.pyramid(tex.image.cpu().numpy(), m.faces.shape[0], 8)
    assert all(np.array_equal(a.image.cpu().numpy(), b[0]) for a, b in zip(pyr.levels, host))
    bg = torch.tensor([0.2, 0.3, 0.4], device=DEV)
    gt = imgs[0][..., :3].to(DEV).float()
    for scale in (1.0, 0.25):
        fr = tr.render_mesh_mip(m, c2w, pyr, background=bg, lod_scale=scale)
        wt = E.render_mesh_mip(m, c2w, tr.K, tr.H, tr.W, pyr, background=bg, near=float(tr.near), lod_scale=scale)
        for a, b in zip(fr, wt):
            assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert fr.rgb.shape == (8, 8, 3) and torch.equal(fr.face, tr.render_mesh(m, c2w, texture=tex).face)
        mse = torch.mean((fr.rgb - gt) ** 2)
        assert tr.mesh_psnr_mip(m, c2w, gt, pyr, background=bg, lod_scale=scale) == float(10.0 * torch.log10(1.0 / mse))


def test_no_faces_on_the_device():
    from nerf_meets_mlx_amd.engine import mesh as E
    v = _dev(S.tetrahedron()[0], torch.float32)
    m = E.Mesh(v, torch.zeros(0, 3, dtype=torch.int32, device=DEV), torch.zeros_like(v), None)
    tex = E.Texture(torch.zeros(10, 10, 3, dtype=torch.uint8, device=DEV), torch.zeros(0, 3, 2, device=DEV), 8)
    stages = []
    pyr = E.build_mipmaps(tex, m, mark=stages.append)
    assert stages == [] and pyr.levels[0] is tex
    assert [tuple(t.image.shape) for t in pyr.levels] == [(10, 10, 3), (6, 6, 3), (4, 4, 3)]
    assert all(t.image.is_cuda and not t.image.any() and t.uv.shape == (0, 3, 2) for t in pyr.levels)
    assert E.face_lod(m, POSES[0], R.intrinsics(5, 6)).shape == (0,)
    rgb = E.sample_texture_mip(pyr, m, _dev([0, -1], torch.int32), torch.zeros(2, 2, device=DEV), torch.zeros(2, device=DEV))
    assert rgb.shape == (2, 3) and not rgb.any()
    bg = torch.tensor([0.25, 0.5, 0.75], device=DEV)
    fr = E.render_mesh_mip(m, POSES[0], R.intrinsics(5, 6), 5, 6, pyr, background=bg)
    assert fr.rgb.shape == (5, 6, 3) and bool((fr.rgb == bg).all()) and bool((fr.face == -1).all())
