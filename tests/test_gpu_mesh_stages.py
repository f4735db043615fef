"""The stage hook of the mesh layer on the GPU (nerf_meets_mlx_amd/engine/mesh): the `mark` sequences that the
docstrings of connected_components, filter_components, erode, reconstruct, _open_components, _simplify, _smooth, rasterize and
project_texture state and no other test pins (tools/ngp_mesh.py times the engine through them), as literal lists; and `extract`
against `mesh_volume` on the volume `extract` builds, bit for bit, with every post-processing keyword set and with none.  A ball
in an R = 8 volume, its marching-cubes mesh, two 16 x 16 cameras, texels = 2."""
import numpy as np
import pytest
import torch

from tests import _camera_ref as CR

pytestmark = pytest.mark.gpu
DEV = "cuda"
R, LO, HI = 8, [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]
RADIUS, ISO = 0.72, 0.1
H = W = 16


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"


@pytest.fixture(scope="module")
def E():
    from nerf_meets_mlx_amd.engine import mesh
    return mesh


def query(rays, z):
    """raw [n, 1, 4] of a ball of radius RADIUS at the origin: sigma = RADIUS - |p|, colours a smooth function of p."""
    p = rays[:, :3] + z * rays[:, 3:6]
    sigma = RADIUS - p.norm(dim=1, keepdim=True)
    return torch.cat([0.5 + 0.5 * torch.sin(3.0 * p), sigma], 1)[:, None, :].contiguous()


@pytest.fixture(scope="module")
def volume(E):
    vol = E.density_volume(query, E.RELU, R, LO, HI, device=DEV)
    inside = int((vol > ISO).sum())
    assert vol.shape == (R, R, R) and inside == 56              # |p| < 2.48 voxels; a core of 8 after one erosion
    return vol


@pytest.fixture(scope="module")
def ball(E, volume):
    mesh = E.marching_cubes(volume, ISO, LO, HI)
    assert mesh.verts.shape[0] > 30 and mesh.faces.shape[0] > 60
    return mesh


@pytest.fixture(scope="module")
def cameras():
    return np.stack([CR.look_at((2.5, 0.4, 0.3)), CR.look_at((-0.5, -2.4, 0.8))]), CR.intrinsics(H, W)


def test_component_stages(E, volume):
    s = []
    E.connected_components(volume, ISO, mark=s.append)
    assert s == ["label", "sizes"]
    s = []
    E.filter_components(volume, ISO, 2, False, None, s.append)
    assert s == ["label", "sizes", "filter"]


def test_opening_stages(E, volume):
    s = []
    core, _ = E.erode(volume, ISO, 1, mark=s.append)
    assert s == ["erode"]
    s = []
    E.reconstruct(volume, core, ISO, 1, mark=s.append)
    assert s == ["reconstruct"]
    s = []
    out = E._open_components(volume, ISO, 1, 2, False, mark=s.append)
    assert s == ["erode", "label", "sizes", "filter", "reconstruct"] and out[2] is not None
    s = []
    out = E._open_components(volume, ISO, 1, mark=s.append)
    assert s == ["erode", "reconstruct"] and out[2] is None


def test_surface_stages(E, ball):
    s = []
    E._simplify(ball, 4, LO, HI, "quadric", False, mark=s.append)
    assert s == ["cluster", "sort", "count", "write"]
    s = []
    E._smooth(ball, 1, LO, HI, 0.5, -0.53, False, mark=s.append)
    assert s == ["build", "run", "normals"]


def test_raster_and_projection_stages(E, ball, cameras):
    c2w, K = cameras
    s = []
    acc = E.rasterize(ball, c2w[0], K, H, W, mark=s.append)[3]
    assert s == ["clear", "draw", "resolve"] and 10 < int(acc.sum()) < H * W
    images = torch.rand(2, H, W, 3, generator=torch.Generator().manual_seed(36)).to(DEV)
    s = []
    tex, seen = E.project_texture(ball, images, c2w, K, texels=2, depth_tol=0.1, mark=s.append)
    assert s == ["rasterize", "rasterize", "accumulate", "finish", "uv"] and int(seen.sum()) > 0 and tex.texels == 2


def _same(a, b):
    assert (a.colors is None) == (b.colors is None)
    for x, y in zip(a, b):
        if x is not None:
            assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_extract_is_mesh_volume_on_its_own_volume(E, volume):
    """With every post-processing keyword set, and with none."""
    post = dict(simplify_grid=4, simplify_placement="quadric", smooth_iterations=1, smooth_lambda=0.5, smooth_mu=-0.53)
    got = E.extract(query, E.RELU, R, ISO, LO, HI, colors=True, device=DEV, opening_radius=1, min_component=2, **post)
    want = E.mesh_volume(query, E.open_components(volume, ISO, 1, 2, False), ISO, LO, HI, True, **post)
    assert got.verts.shape[0] > 3 and got.faces.shape[0] > 3 and got.colors is not None
    _same(got, want)
    plain = E.extract(query, E.RELU, R, ISO, LO, HI, colors=True, device=DEV)
    assert plain.verts.shape[0] > got.verts.shape[0]
    _same(plain, E.mesh_volume(query, volume, ISO, LO, HI, True))
