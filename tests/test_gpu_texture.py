"""The texture atlas on the GPU (csrc/texture.hip, engine/mesh/texture.py bake_texture / sample_texture, Trainer.texture_mesh) against
the numpy reference of tests/_texture_ref.py: row, image, UV and sampler bits compared as integers -- no tolerance, the rule is
exact -- into sentinel-filled outputs; chunked stores into a poisoned image; bad faces and zero normals; and the
functional property the layout exists for: a bilinear lookup never reads another face's texels."""
import numpy as np
import pytest
import torch

from tests import _smooth_ref as S
from tests import _texture_ref as T
from tests._poison import bits_equal, sentinel_, unwritten

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL = 0xA5                                                            # what the image holds before a store


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


def _mesh(name):
    from nerf_meets_mlx_amd.engine import mesh as E
    v, f = MESHES[name]()
    n = T.vertex_normals(v, f)
    return (np.asarray(v), np.asarray(f), n), E.Mesh(_dev(v, torch.float32), _dev(f, torch.int32), _dev(n, torch.float32))


def _raw_for(P, seed):
    """raw [P, 4] with values below 0, above 1, ties of rint, NaN and infinities among ordinary ones."""
    rng = np.random.default_rng(seed)
    raw = rng.uniform(-0.2, 1.2, (P, 4)).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, 0.5 / 255, 1.5 / 255, 2.5 / 255, 1.0, 0.0, -0.0, 254.5 / 255], np.float32)
    idx = rng.integers(0, P * 4, min(P, 64))
    raw.reshape(-1)[idx] = special[rng.integers(0, len(special), len(idx))]
    return raw


def _c_rows(mesh, texels, p0, count, spare=1):
    from nerf_meets_mlx_amd import _native as N
    out = sentinel_(torch.empty(count + spare, 11, dtype=torch.float32, device=DEV))
    N.check(N.lib().nerf_texture_rows(N.ptr(mesh.verts), N.ptr(mesh.normals), mesh.verts.shape[0], N.ptr(mesh.faces), mesh.faces.shape[0],
                                      texels, p0, count, N.ptr(out), N.stream()))
    assert unwritten(out[count:]) == 11 * spare and unwritten(out[:count]) == 0
    return out[:count]


def _c_store(mesh, texels, raw_all, chunk):
    """nerf_texture_store chunk by chunk; the raw buffer is NaN before each chunk's values are copied in, the image holds FILL."""
    from nerf_meets_mlx_amd import _native as N
    W, H = T.layout(mesh.faces.shape[0], texels)[:2]
    image = torch.full((H * W * 3 + 4,), FILL, dtype=torch.uint8, device=DEV)
    raw = torch.empty(chunk, 4, dtype=torch.float32, device=DEV)
    src = _dev(raw_all, torch.float32)
    for p0 in range(0, W * H, chunk):
        cnt = min(chunk, W * H - p0)
        raw.fill_(float("nan"))
        raw[:cnt] = src[p0:p0 + cnt]
        N.check(N.lib().nerf_texture_store(N.ptr(raw), mesh.verts.shape[0], N.ptr(mesh.faces), mesh.faces.shape[0], texels, p0, cnt,
                                           N.ptr(image), N.stream()))
    assert bool((image[H * W * 3:] == FILL).all())                     # nothing is written behind the image
    return image[:H * W * 3].view(H, W, 3)


# ------------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("texels", [2, 3, 8])
@pytest.mark.parametrize("name,F", [("tetrahedron", 4), ("sphere12", 768), ("sphere24", 4064), ("soup37", 37)])
def test_kernels_match_the_reference_bit_for_bit(name, F, texels):
    from nerf_meets_mlx_amd import _native as N
    from nerf_meets_mlx_amd.engine import mesh as E
    (v, f, n), mesh = _mesh(name)
    assert len(f) == F
    W, H, _, Sn = T.layout(F, texels)
    P = W * H
    # rows: the whole atlas in one call, and a chunk that starts and ends inside a workgroup's span
    want = T.texel_rows(v, n, f, texels)
    got = _c_rows(mesh, texels, 0, P).cpu().numpy()
    bad = (_bits(got) != _bits(want)).any(1)
    assert not bad.any(), ("row bits differ", int(bad.sum()), np.nonzero(bad)[0][:4], got[bad][:2], want[bad][:2])
    p0, cnt = min(P - 1, 259), min(P - min(P - 1, 259), 300)
    assert np.array_equal(_bits(_c_rows(mesh, texels, p0, cnt).cpu().numpy()), _bits(want[p0:p0 + cnt]))
    # image: chunks of 1001 texels, which end inside a wave
    raw = _raw_for(P, texels)
    want_img = T.store(raw, f, len(v), texels)
    got_img = _c_store(mesh, texels, raw, 1001).cpu().numpy()
    assert np.array_equal(got_img, want_img), np.argwhere((got_img != want_img).any(2))[:4]
    Y, X = np.mgrid[0:H, 0:W]
    unused = (T.owner((W, H, W // Sn, Sn), X, Y)[0] >= F)
    assert unused.sum() == P - sum(Sn * (Sn + 1) // 2 if k % 2 == 0 else Sn * (Sn - 1) // 2 for k in range(F))
    assert not got_img[unused].any() and got_img[~unused].any()
    # uv
    uv = sentinel_(torch.empty(F + 1, 3, 2, dtype=torch.float32, device=DEV))
    N.check(N.lib().nerf_texture_uv(F, texels, N.ptr(uv), N.stream()))
    assert unwritten(uv[F:]) == 6 and np.array_equal(_bits(uv[:F].cpu().numpy()), _bits(T.uvs(F, texels)))
    # sampler: corners, edges, points outside the triangle, NaN, faces outside [0, F)
    rng = np.random.default_rng(F + texels)
    ns = 1500
    sf = rng.integers(0, F, ns).astype(np.int32)
    sf[:8] = [-1, F, F + 1, -2 ** 31, 2 ** 31 - 1, 0, F - 1, F - 1]
    sb = rng.dirichlet([1, 1, 1], ns)[:, 1:].astype(np.float32)
    sb[8:20] = [[0, 0], [1, 0], [0, 1], [0.5, 0.5], [0.5, 0], [0, 0.5], [-0.5, 0.5], [0.7, 0.7], [np.nan, 0.5], [0.5, np.nan], [2, 2], [1, 1]]
    tex = E.Texture(_dev(want_img, torch.uint8), uv[:F].clone(), texels)
    tf, tb = _dev(sf, torch.int32), _dev(sb, torch.float32)
    rgb, rows = E.sample_texture(tex, mesh, tf, tb, rows=True)
    wrgb, wrows = T.sample(want_img, v, n, f, texels, sf, sb, rows=True)
    assert np.array_equal(_bits(rgb.cpu().numpy()), _bits(wrgb)) and np.array_equal(_bits(rows.cpu().numpy()), _bits(wrows))
    assert not wrgb[:5].any() and not wrows[:5].any() and wrgb.any()
    assert bits_equal(E.sample_texture(tex, mesh, tf, tb), rgb)           # without rows: the same colours


# ------------------------------------------------------------------------------------------------ chunks and repeats
def _query(rows, z):
    raw = torch.zeros(rows.shape[0], 1, 4, dtype=torch.float32, device=rows.device)
    raw[:, 0, :3] = 0.5 + 0.6 * torch.sin(3.0 * rows[:, :3] + rows[:, 3:6])
    return raw


@pytest.mark.parametrize("name,texels", [("tetrahedron", 3), ("soup37", 3), ("soup37", 8)])
def test_the_image_does_not_depend_on_the_chunk_and_two_runs_agree(name, texels):
    from nerf_meets_mlx_amd.engine import mesh as E
    (v, f, n), mesh = _mesh(name)
    W, H = T.layout(len(f), texels)[:2]
    calls = []

    def query(rows, z):
        assert z.shape == (rows.shape[0], 1) and not z.any()
        calls.append(rows.shape[0])
        return _query(rows, z)
    whole = E.bake_texture(query, mesh, texels)
    assert calls == [W * H] and whole.image.shape == (H, W, 3) and whole.texels == texels
    want = T.bake(lambda r: _query(_dev(r, torch.float32), None).reshape(-1, 4).cpu().numpy(), v, n, f, texels)
    assert np.array_equal(whole.image.cpu().numpy(), want[0]) and np.array_equal(_bits(whole.uv.cpu().numpy()), _bits(want[1]))
    for chunk in (1, 7, W + 1, W * H, 1 << 19):
        del calls[:]
        t = E.bake_texture(query, mesh, texels, chunk=chunk)
        assert len(calls) == -(-W * H // min(chunk, W * H)) and sum(calls) == W * H
        assert torch.equal(t.image, whole.image) and bits_equal(t.uv, whole.uv), chunk
    again = E.bake_texture(query, mesh, texels)
    assert torch.equal(again.image, whole.image) and bits_equal(again.uv, whole.uv)
    stages = []
    E.bake_texture(query, mesh, texels, chunk=W * H // 2 + 1, mark=stages.append)
    assert stages == ["rows", "query", "store"] * 2 + ["uv"]
    with pytest.raises(ValueError, match="the query must return"):       # a short answer never reaches the store
        E.bake_texture(lambda rows, z: _query(rows[:-1], z), mesh, texels)


# ------------------------------------------------------------------------------------------------ bad faces, zero normals
def test_bad_faces_give_zero_rows_and_black_texels():
    from nerf_meets_mlx_amd.engine import mesh as E
    v, f = S.sphere(12)
    f = f[:101].copy()                                                    # odd: the last cell is half used
    V = len(v)
    f[3, 1], f[10, 0], f[11, 2], f[100, 0] = V, -1, np.iinfo(np.int32).max, np.iinfo(np.int32).min
    n = T.vertex_normals(v, np.where((f >= 0) & (f < V), f, 0))
    mesh = E.Mesh(_dev(v, torch.float32), _dev(f, torch.int32), _dev(n, torch.float32))
    texels = 3
    W, H, Cn, Sn = T.layout(len(f), texels)
    got = _c_rows(mesh, texels, 0, W * H).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(T.texel_rows(v, n, f, texels)))
    Y, X = np.mgrid[0:H, 0:W]
    own = T.owner((W, H, Cn, Sn), X.ravel(), Y.ravel())[0]
    bad = np.isin(own, [3, 10, 11, 100])
    assert bad.sum() == 2 * Sn * (Sn - 1) // 2 + 2 * Sn * (Sn + 1) // 2
    assert not _bits(got[bad]).any() and np.abs(got[~bad & (own < len(f))][:, :3]).sum(1).all()
    raw = np.full((W * H, 4), 0.7, np.float32)
    img = _c_store(mesh, texels, raw, 13).cpu().numpy().reshape(-1, 3)
    assert np.array_equal(img.reshape(H, W, 3), T.store(raw, f, V, texels))
    assert not img[bad].any() and (img[~bad & (own < len(f))] == 178).all()
    sf = _dev([3, 10, 11, 100, 4], torch.int32)
    tex = E.Texture(_dev(img.reshape(H, W, 3), torch.uint8), torch.zeros(len(f), 3, 2, device=DEV), texels)
    rgb, rows = E.sample_texture(tex, mesh, sf, torch.full((5, 2), 0.25, device=DEV), rows=True)
    assert not rgb[:4].any() and not rows[:4].view(torch.int32).any() and rgb[4].all() and rows[4, :3].any()


def test_zero_normals_give_zero_directions():
    from nerf_meets_mlx_amd.engine import mesh as E
    v, f = S.tetrahedron()
    n = T.vertex_normals(v, f)
    n[0] = 0.0                                                            # one corner without a normal: its share is dropped
    some = E.Mesh(_dev(v, torch.float32), _dev(f, torch.int32), _dev(n, torch.float32))
    none = some._replace(normals=torch.zeros_like(some.normals))
    opposite = some._replace(normals=_dev(np.array([[1, 0, 0], [-1, 0, 0], [0, 0, 0], [0, 0, 0]]), torch.float32))
    W, H = T.layout(4, 4)[:2]
    for mesh, nn in ((some, n), (none, np.zeros_like(n)), (opposite, opposite.normals.cpu().numpy())):
        got = _c_rows(mesh, 4, 0, W * H).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(T.texel_rows(v, nn, f, 4)))
    rows = _c_rows(none, 4, 0, W * H).cpu().numpy()
    assert not rows[:, 3:11].any() and rows[:, :3].any()
    # face 0 = (0, 1, 2): halfway between the corners with opposite normals the sum vanishes, the direction is 0, not NaN
    rgb, r = E.sample_texture(E.Texture(torch.zeros(H, W, 3, dtype=torch.uint8, device=DEV), torch.zeros(4, 3, 2, device=DEV), 4), opposite,
                              _dev([0], torch.int32), _dev([[0.5, 0.0]], torch.float32), rows=True)
    assert not r[0, 3:].any() and torch.isfinite(r).all()


# ------------------------------------------------------------------------------------------------ no bleeding
AFFINE_M = np.array([[0.1, 0.05, -0.08], [-0.06, 0.1, 0.07], [0.04, -0.09, 0.1]])
AFFINE_C = np.array([0.5, 0.42, 0.3])


@pytest.mark.parametrize("texels", [2, 3, 8])
def test_a_bilinear_lookup_never_reads_another_faces_texels(texels):
    """sphere24 with its faces permuted at random: atlas neighbours are far apart in space, so a texel read from the wrong face
    would be off by much more than the bound.  The colour is affine in position with values inside [0.1, 0.9]; gutters are
    extrapolated in the face's plane, so a bilinear lookup reproduces it up to 0.5 / 255 (a convex combination of bytes, each
    rounded by at most half a step) + 1e-5 (float32 rounding of the field, the weights and the sum)."""
    from nerf_meets_mlx_amd.engine import mesh as E
    v, f = S.sphere(24)
    f = f[np.random.default_rng(24).permutation(len(f))]
    mesh = E.Mesh(_dev(v, torch.float32), _dev(f, torch.int32), _dev(T.vertex_normals(v, f), torch.float32))
    M32, c32 = _dev(AFFINE_M, torch.float32), _dev(AFFINE_C, torch.float32)

    def query(rows, z):
        raw = torch.ones(rows.shape[0], 1, 4, dtype=torch.float32, device=rows.device)
        raw[:, 0, :3] = rows[:, :3] @ M32.T + c32
        return raw
    tex = E.bake_texture(query, mesh, texels)
    rng = np.random.default_rng(texels)
    fixed = np.array([[0, 0], [1, 0], [0, 1], [0.5, 0], [0, 0.5], [0.5, 0.5]])
    F = len(f)
    bary = np.concatenate([np.broadcast_to(fixed, (F, 6, 2)), rng.dirichlet([1, 1, 1], (F, 50))[:, :, 1:]], 1).astype(np.float32)
    face = np.repeat(np.arange(F, dtype=np.int32), bary.shape[1])
    rgb, rows = E.sample_texture(tex, mesh, _dev(face, torch.int32), _dev(bary.reshape(-1, 2), torch.float32), rows=True)
    want = rows[:, :3].cpu().numpy().astype(np.float64) @ AFFINE_M.T + AFFINE_C
    assert 0.1 <= want.min() and want.max() <= 0.9
    err = np.abs(rgb.cpu().numpy().astype(np.float64) - want).max()
    print("texels", texels, "max |lookup - field|", err, "bound", 0.5 / 255 + 1e-5)
    assert err <= 0.5 / 255 + 1e-5
    # the sampled points are the faces' own: corner a of every face is vertex a
    assert bits_equal(rows[0::56, :3], mesh.verts[mesh.faces[:, 0].long()])


# ------------------------------------------------------------------------------------------------ trainer, empty mesh
def test_trainer_texture_mesh_is_bake_texture_of_its_field():
    from nerf_meets_mlx_amd.dataset import synthetic
    from nerf_meets_mlx_amd.engine import mesh as E
    from nerf_meets_mlx_amd.engine.trainer import Trainer
    imgs, poses, _, _, K = synthetic.make_dataset(8, 8, 2, seed=0, device=DEV)
    tr = Trainer(imgs, poses, K, N_rand=64, n_depth_samples=16, N_importance=16, seed=4, device=DEV)
    box = ([-1.0] * 3, [1.0] * 3)
    vol = tr.density_volume(16, box)
    thr = float(vol.reshape(-1).quantile(0.7))
    m = tr.extract_mesh(resolution=16, threshold=thr, aabb=box)
    F = m.faces.shape[0]
    print("V, F", m.verts.shape[0], F)
    assert F > 0
    tex = tr.texture_mesh(m, texels=4)
    want = E.bake_texture(tr._mesh_field()[0], m, 4)
    W, H = E.texture_layout(F, 4)[:2]
    assert tex.image.shape == (H, W, 3) and tex.uv.shape == (F, 3, 2) and tex.texels == 4
    assert torch.equal(tex.image, want.image) and bits_equal(tex.uv, want.uv) and tex.image.any()
    assert torch.equal(tr.texture_mesh(m).image, E.bake_texture(tr._mesh_field()[0], m, 8).image)
    with pytest.raises(ValueError):
        tr.texture_mesh(m, texels=1)


def test_no_faces_on_the_device():
    from nerf_meets_mlx_amd.engine import mesh as E
    v = _dev(S.tetrahedron()[0], torch.float32)
    m = E.Mesh(v, torch.zeros(0, 3, dtype=torch.int32, device=DEV), torch.zeros_like(v))

    def query(rows, z):
        raise AssertionError("queried")
    tex = E.bake_texture(query, m, 8)
    assert tex.image.shape == (10, 10, 3) and tex.image.is_cuda and not tex.image.any() and tex.uv.shape == (0, 3, 2)
    rgb = E.sample_texture(tex, m, _dev([0, -1], torch.int32), torch.zeros(2, 2, device=DEV))
    assert rgb.shape == (2, 3) and not rgb.any()
