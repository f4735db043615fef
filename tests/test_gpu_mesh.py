"""Mesh extraction on the GPU (csrc/mesh.hip, engine/mesh, Trainer.density_volume / extract_mesh) against the numpy reference
of tests/_mesh_ref.py: vertices and faces bit for bit (normals within 1e-6) at lattice sizes that are no multiple of a workgroup,
with iso values present in the volume, NaN / +-inf corners and constant volumes, into poisoned buffers; reproducibility; the
density volume against the fields' query of torch-built lattice rows; the vertex colours; a march-mode trainer's mesh through
write_ply."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _mesh_ref as M
from tests._poison import NAN_BYTES, PATTERNS, bits_equal, poison_, sentinel_, unwritten

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT32 = 0x7FE5A5A5


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"


def _volume(R, kind, seed=0):
    rng = np.random.default_rng(seed + R)
    x = (np.arange(R) + 0.5) / R * 2 - 1
    Z, Y, X = np.meshgrid(x, x, x, indexing="ij")
    v = (0.6 - np.sqrt(X * X + 1.3 * Y * Y + 0.8 * Z * Z) + 0.05 * rng.standard_normal((R, R, R))).astype(np.float32)
    if kind == "quantised":                                   # many corners exactly at the iso level 0
        v = np.round(v * 8) / 8
    elif kind == "special":                                   # NaN and +-inf corners, exact iso hits
        flat = v.reshape(-1)
        idx = rng.permutation(flat.size)
        k = max(1, flat.size // 20)
        flat[idx[:k]] = np.nan
        flat[idx[k:2 * k]] = np.inf
        flat[idx[2 * k:3 * k]] = -np.inf
        flat[idx[3 * k:4 * k]] = 0.0
    elif kind == "noise":
        v = rng.standard_normal((R, R, R)).astype(np.float32)
    return np.ascontiguousarray(v, dtype=np.float32)


def _mc_poisoned(vol, iso, lo, hi, pattern):
    """The C calls of engine.mesh.marching_cubes with sentinel outputs and a poisoned workspace; (verts, faces, normals, rows)."""
    from nerf_meets_mlx_amd import _native as N
    L = N.lib()
    R = vol.shape[0]
    clo, chi = (C.c_float * 3)(*lo), (C.c_float * 3)(*hi)
    ws = poison_(torch.empty(L.nerf_mesh_workspace_bytes(R), dtype=torch.uint8, device=DEV), pattern)
    tot = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    N.check(L.nerf_mesh_count(N.ptr(vol), R, float(iso), N.ptr(ws), N.ptr(tot), N.stream()))
    V, F = tot.tolist()
    verts = sentinel_(torch.empty(V + 1, 3, dtype=torch.float32, device=DEV))       # one spare row: nothing is written past V
    normals = sentinel_(torch.empty(V + 1, 3, dtype=torch.float32, device=DEV))
    rows = sentinel_(torch.empty(V + 1, 11, dtype=torch.float32, device=DEV))
    faces = torch.full((F + 1, 3), SENT32, dtype=torch.int32, device=DEV)
    N.check(L.nerf_mesh_write_vertices(N.ptr(vol), R, float(iso), clo, chi, N.ptr(ws), V, N.ptr(verts), N.ptr(normals),
                                       N.ptr(rows), N.stream()))
    N.check(L.nerf_mesh_write_faces(N.ptr(vol), R, float(iso), N.ptr(ws), F, N.ptr(faces), N.stream()))
    torch.cuda.synchronize()
    assert unwritten(verts[V:]) == 3 and unwritten(normals[V:]) == 3 and unwritten(rows[V:]) == 11
    assert bool((faces[F:] == SENT32).all())
    return verts[:V], faces[:F], normals[:V], rows[:V]


def _check_against_reference(v, iso, lo, hi):
    vol = torch.from_numpy(v).to(DEV)
    wv, wf, wn = M.marching_cubes(v, iso, lo, hi)
    for pattern in PATTERNS:
        verts, faces, normals, rows = _mc_poisoned(vol, iso, lo, hi, pattern)
        assert unwritten(verts) == 0 and unwritten(normals) == 0 and unwritten(rows) == 0
        assert verts.shape == wv.shape and faces.shape == wf.shape
        assert bits_equal(verts.cpu(), torch.from_numpy(wv))
        assert torch.equal(faces.cpu(), torch.from_numpy(wf))
        assert float((normals.cpu() - torch.from_numpy(wn)).abs().max()) <= 1e-6 if len(wn) else True
        # colour rows [x, -n, 0, 0, -n]
        want_rows = torch.cat([verts, -normals, torch.zeros(len(verts), 2, device=DEV), -normals], 1)
        assert bits_equal(rows, want_rows)
    from nerf_meets_mlx_amd.engine.mesh import marching_cubes
    m = marching_cubes(vol, iso, lo, hi)
    assert bits_equal(m.verts.cpu(), torch.from_numpy(wv)) and torch.equal(m.faces.cpu(), torch.from_numpy(wf))
    return wv, wf


@pytest.mark.parametrize("R", [2, 3, 17, 64, 65, 130])
@pytest.mark.parametrize("kind", ["smooth", "quantised", "special"])
def test_marching_cubes_matches_the_reference_bit_for_bit(R, kind):
    v = _volume(R, kind)
    lo, hi = [-1.1, -0.7, 0.3], [0.9, 1.6, 2.05]
    wv, wf = _check_against_reference(v, 0.0, lo, hi)
    if kind == "smooth" and R >= 17:
        assert len(wf) > 0 and M.closed_and_oriented(wf)


@pytest.mark.parametrize("R", [3, 65])
def test_noise_and_constant_volumes(R):
    _check_against_reference(_volume(R, "noise"), 0.25, [0, 0, 0], [1, 1, 1])
    const = np.full((R, R, R), 2.0, np.float32)
    for iso in (2.0, 1.0, 3.0):                               # v == iso is outside: V = F = 0 every time
        wv, wf = _check_against_reference(const, iso, [0, 0, 0], [1, 1, 1])
        assert len(wv) == 0 and len(wf) == 0


def test_two_calls_are_bit_identical():
    from nerf_meets_mlx_amd.engine.mesh import marching_cubes
    vol = torch.from_numpy(_volume(130, "special")).to(DEV)
    a = marching_cubes(vol, 0.0, [-1] * 3, [1] * 3)
    b = marching_cubes(vol, 0.0, [-1] * 3, [1] * 3)
    assert bits_equal(a.verts, b.verts) and torch.equal(a.faces, b.faces) and bits_equal(a.normals, b.normals)


# ------------------------------------------------------------------------------------------------ density volume
def _hash_field(seed=3):
    from nerf_meets_mlx_amd.engine.ngp import HashNeRF
    f = HashNeRF(device=DEV, seed=seed, log2_hashmap_size=14)
    f.enc.tables.normal_(0.0, 0.3, generator=torch.Generator(device=DEV).manual_seed(seed))
    return f


def _torch_rows(R, lo, hi):
    """Lattice rows built with torch ops in the stated order: p_a = lo_a + ((float)i_a + 0.5f) * h_a."""
    lo32 = torch.tensor(lo, dtype=torch.float32, device=DEV)
    h = (torch.tensor(hi, dtype=torch.float32, device=DEV) - lo32) / torch.tensor(float(R), dtype=torch.float32, device=DEV)
    i = torch.arange(R, dtype=torch.float32, device=DEV) + 0.5
    ax = [lo32[a] + i * h[a] for a in range(3)]
    k, j, ii = torch.meshgrid(torch.arange(R, device=DEV), torch.arange(R, device=DEV), torch.arange(R, device=DEV), indexing="ij")
    p = torch.stack([ax[0][ii], ax[1][j], ax[2][k]], -1).reshape(-1, 3)
    rows = torch.cat([p, torch.zeros(p.shape[0], 8, device=DEV)], 1).contiguous()
    return rows, torch.zeros(p.shape[0], 1, device=DEV)


def _merge(raw, act):
    from nerf_meets_mlx_amd import _native as N
    out = torch.zeros(raw.shape[0], dtype=torch.float32, device=DEV)
    raw = raw.reshape(-1, 4).contiguous()
    N.check(N.lib().nerf_occ_merge_ex(N.ptr(out), N.ptr(raw), raw.shape[0], 0.0, act, N.stream()))
    return out


def _check_volume(query, act, R, lo, hi):
    from nerf_meets_mlx_amd.engine import mesh
    vol = mesh.density_volume(query, act, R, lo, hi, device=DEV)
    rows, z = _torch_rows(R, lo, hi)
    from nerf_meets_mlx_amd.engine.mesh import lattice_rows
    r2, z2 = lattice_rows(R, lo, hi, device=DEV)
    assert bits_equal(r2, rows) and bits_equal(z2, z)
    s = query(rows, z).reshape(-1, 4)[:, 3]
    if act == mesh.RELU:
        want = torch.where(s > 0, s, torch.zeros_like(s))
        assert bits_equal(vol.reshape(-1), want)
    else:
        assert bits_equal(vol.reshape(-1), _merge(query(rows, z), act))
        ref = torch.where(torch.isnan(s), torch.zeros_like(s), torch.exp(s))
        ulp = (vol.reshape(-1).view(torch.int32).long() - ref.view(torch.int32).long()).abs()
        assert int(ulp.max()) <= 1                            # device expf vs torch's exp
    # the volume does not depend on the query chunk
    small = mesh.density_volume(query, act, R, lo, hi, device=DEV, chunk=4099)
    assert bits_equal(small, vol)
    return vol


@pytest.mark.parametrize("act", [0, 1])
def test_density_volume_of_the_hash_grid_field(act):
    f = _hash_field()
    _check_volume(lambda r, z: f.query(r, z), act, 33, [-1.5] * 3, [1.5] * 3)


def test_density_volume_of_the_8x256_field():
    from nerf_meets_mlx_amd.models.NeRF import NeRF
    m = NeRF(channel_input=63, channel_input_views=27, is_use_view_directions=True, device=DEV, seed=0)
    _check_volume(lambda r, z: m.query(r, z), 0, 19, [-1.2, -1.0, -0.8], [1.2, 1.1, 0.9])


def test_vertex_colours_are_the_clamped_field_along_minus_normal():
    from nerf_meets_mlx_amd.engine import mesh
    f = _hash_field(5)
    q = lambda r, z: f.query(r, z)
    vol = mesh.density_volume(q, mesh.RELU, 40, [-1.5] * 3, [1.5] * 3, device=DEV)
    iso = float(vol.reshape(-1).median())
    m = mesh.extract(q, mesh.RELU, 40, iso, [-1.5] * 3, [1.5] * 3, colors=True, device=DEV)
    assert m.faces.shape[0] > 0 and m.colors.shape == m.verts.shape
    n = m.normals
    rows = torch.cat([m.verts, -n, torch.zeros(len(n), 2, device=DEV), -n], 1).contiguous()
    want = f.query(rows, torch.zeros(len(n), 1, device=DEV)).reshape(-1, 4)[:, :3].clamp(0.0, 1.0)
    assert bits_equal(m.colors, want)
    assert float(m.colors.min()) >= 0.0 and float(m.colors.max()) <= 1.0
    plain = mesh.extract(q, mesh.RELU, 40, iso, [-1.5] * 3, [1.5] * 3, colors=False, device=DEV)
    assert plain.colors is None and bits_equal(plain.verts, m.verts) and torch.equal(plain.faces, m.faces)


# ------------------------------------------------------------------------------------------------ trainers
def _small_images(hw, views):
    from nerf_meets_mlx_amd.dataset import synthetic
    return synthetic.make_dataset(hw, hw, views, seed=0, device=DEV)


def test_trainer_density_volume_uses_the_fine_network_and_needs_a_box():
    from nerf_meets_mlx_amd.engine.mesh import RELU
    from nerf_meets_mlx_amd.engine.trainer import Trainer
    imgs, poses, _, _, K = _small_images(8, 2)
    tr = Trainer(imgs, poses, K, N_rand=64, n_depth_samples=16, N_importance=16, seed=4, device=DEV)
    with pytest.raises(ValueError):
        tr.density_volume(8)
    box = ([-1.0, -1.0, -1.0], [1.0, 1.0, 1.0])
    vol = tr.density_volume(21, box)
    want = _check_volume(lambda r, z: tr.fine.query(r, z, ref_quirks=tr.q), RELU, 21, *box)
    assert bits_equal(vol, want)
    coarse_only = Trainer(imgs, poses, K, N_rand=64, n_depth_samples=16, N_importance=0, seed=4, device=DEV)
    assert bits_equal(coarse_only.density_volume(9, box),
                      _check_volume(lambda r, z: coarse_only.coarse.query(r, z), RELU, 9, *box))


def test_ngp_trainer_density_volume_activation_and_box():
    from nerf_meets_mlx_amd.engine.mesh import EXP, RELU
    from nerf_meets_mlx_amd.engine.ngp import NGPTrainer
    imgs, poses, _, _, K = _small_images(8, 2)
    plain = NGPTrainer(imgs, poses, K, N_rand=64, n_depth_samples=64, seed=4, device=DEV, log2_hashmap_size=14)
    march = NGPTrainer(imgs, poses, K, N_rand=64, n_depth_samples=64, seed=4, device=DEV, log2_hashmap_size=14,
                       occupancy_grid=True, march_steps=256)
    box = ([-1.5] * 3, [1.5] * 3)
    assert bits_equal(plain.density_volume(17), _check_volume(lambda r, z: plain.field.query(r, z), RELU, 17, *box))
    assert bits_equal(march.density_volume(17), _check_volume(lambda r, z: march.field.query(r, z), EXP, 17, *box))
    nobox = NGPTrainer(imgs, poses, K, N_rand=64, n_depth_samples=64, seed=4, device=DEV, log2_hashmap_size=14, bound=None)
    with pytest.raises(ValueError):
        nobox.extract_mesh(8)
    assert nobox.density_volume(5, ([-1] * 3, [1] * 3)).shape == (5, 5, 5)


def test_march_trainer_extract_mesh_and_ply(tmp_path):
    """hw 48, 2^14-entry tables, march mode (test_gpu_march.py's fixture), past the grid's warm-up."""
    from nerf_meets_mlx_amd.engine.mesh import read_ply, write_ply
    from nerf_meets_mlx_amd.engine.ngp import NGPTrainer
    imgs, poses, _, _, K = _small_images(48, 8)
    tr = NGPTrainer(imgs, poses, K, N_rand=256, n_depth_samples=64, seed=4, device=DEV, log2_hashmap_size=14,
                    occupancy_grid=True, march_steps=1024)
    for _ in range(300):
        tr.train_step()
    vol = tr.density_volume(64)
    thr = float(vol.reshape(-1).quantile(0.9))
    assert float(vol.min()) < thr < float(vol.max())
    a = tr.extract_mesh(64, threshold=thr)
    b = tr.extract_mesh(64, threshold=thr)
    V, F = a.verts.shape[0], a.faces.shape[0]
    assert V > 0 and F > 0
    assert bits_equal(a.verts, b.verts) and torch.equal(a.faces, b.faces) and bits_equal(a.normals, b.normals)
    assert bits_equal(a.colors, b.colors)
    assert bool((a.verts > -1.5).all()) and bool((a.verts < 1.5).all())
    assert int(a.faces.min()) >= 0 and int(a.faces.max()) < V
    wv, wf, _ = M.marching_cubes(vol.cpu().numpy(), thr, [-1.5] * 3, [1.5] * 3)
    assert bits_equal(a.verts.cpu(), torch.from_numpy(wv)) and torch.equal(a.faces.cpu(), torch.from_numpy(wf))
    p = write_ply(str(tmp_path / "ngp.ply"), a)
    back = read_ply(p)
    assert bits_equal(back.verts, a.verts.cpu()) and torch.equal(back.faces, a.faces.cpu())
    assert bits_equal(back.normals, a.normals.cpu())
    assert torch.equal(torch.round(back.colors * 255), torch.round(a.colors.cpu().double() * 255).float())
    d = M.directed_edges(back.faces.numpy())
    assert len(np.unique(d[:, 0] * V + d[:, 1])) == len(d)      # every directed edge at most once: consistently oriented
