"""Connected components on the GPU (csrc/ccl.hip, engine/mesh/volume.py connected_components / filter_components, extract_mesh's
min_component / largest_only) against the reference of tests/_ccl_ref.py: labels, sizes, stats and filtered volumes bit for bit,
into sentinel outputs with one spare element and a poisoned workspace, at lattice sizes that are no multiple of a wave or a
workgroup, on the volumes a labelling kernel goes wrong on; reproducibility; the filter through marching cubes; a march-mode
trainer's filtered mesh through write_ply."""
import functools

import numpy as np
import pytest
import torch

from tests import _ccl_ref as CC
from tests import _mesh_ref as M
from tests._poison import PATTERNS, bits_equal, poison_

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT32 = 0x7FE5A5A5
SENT64 = 0x7FE5A5A57FE5A5A5
SIZES = [2, 3, 17, 64, 65]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"


# ------------------------------------------------------------------------------------------------ volumes
def _centres(R):
    x = (np.arange(R) + 0.5) / R * 2 - 1
    return np.meshgrid(x, x, x, indexing="ij")                       # Z, Y, X


def _serpentine(R):
    """One voxel-wide path through every second row of every second layer: along x, a step in y, back along x, ..., then up in z
    at the end of the layer and back: one component whose longest path is about R^3 / 2 voxels."""
    v = np.zeros((R, R, R), np.float32)
    path = []
    j_fwd = True
    for k in range(0, R, 2):
        js = list(range(0, R, 2)) if j_fwd else list(range(R - 1 - (R - 1) % 2, -1, -2))
        for n, j in enumerate(js):
            fwd = (len(path) == 0) or path[-1][2] == 0
            path += [(k, j, i) for i in (range(R) if fwd else range(R - 1, -1, -1))]
            if n + 1 < len(js):
                path.append((k, (j + js[n + 1]) // 2, path[-1][2]))
        if k + 2 < R:
            path.append((k + 1, path[-1][1], path[-1][2]))
        j_fwd = not j_fwd
    for s, (k, j, i) in enumerate(path):
        v[k, j, i] = 1.0 + (s % 7)
    for a, b in zip(path[:-1], path[1:]):
        assert sum(abs(p - q) for p, q in zip(a, b)) == 1
    return v


@functools.lru_cache(maxsize=None)
def _case(kind, R):
    """(volume float32 [R, R, R], iso, reference (labels, sizes, stats)) -- computed once per module run, never changed."""
    rng = np.random.default_rng(100 + R)
    iso = 0.0
    if kind in ("noise", "noise75"):
        v = rng.standard_normal((R, R, R)).astype(np.float32)
        if kind == "noise75":
            iso = float(np.quantile(v, 0.75))
    elif kind == "checkerboard":
        k, j, i = np.indices((R, R, R))
        v, iso = ((i + j + k) % 2 == 0).astype(np.float32), 0.5
    elif kind == "serpentine":
        v, iso = _serpentine(R), 0.5
    elif kind == "row_ends":                                         # i = R - 1 and i = 0 everywhere: two sheets, never joined
        v, iso = np.zeros((R, R, R), np.float32), 0.5
        v[:, :, 0] = 1.0
        v[:, :, R - 1] = 2.0
    elif kind == "row_end_pairs":                                    # (i = R - 1, j) and (i = 0, j + 1) for even j and k: all single
        v, iso = np.zeros((R, R, R), np.float32), 0.5
        v[0::2, 0:R - 1:2, R - 1] = 1.0
        v[0::2, 1:R:2, 0] = 1.0
    elif kind == "all_inside":
        v, iso = np.full((R, R, R), 2.0, np.float32), 1.0
    elif kind == "all_outside":
        v, iso = np.full((R, R, R), 2.0, np.float32), 2.0            # v == iso is outside
    elif kind == "special":                                          # test_gpu_mesh.py's: NaN, +-inf and exact-iso voxels
        Z, Y, X = _centres(R)
        v = (0.6 - np.sqrt(X * X + 1.3 * Y * Y + 0.8 * Z * Z) + 0.05 * rng.standard_normal((R, R, R))).astype(np.float32)
        flat = v.reshape(-1)
        idx = rng.permutation(flat.size)
        n = max(1, flat.size // 20)
        flat[idx[:n]] = np.nan
        flat[idx[n:2 * n]] = np.inf
        flat[idx[2 * n:3 * n]] = -np.inf
        flat[idx[3 * n:4 * n]] = 0.0
        flat.view(np.uint32)[idx[:n:2]] = 0x7FC12345                 # NaNs with a payload
    elif kind == "shell":                                            # one component around an outside cavity with a speck in it
        Z, Y, X = _centres(R)
        r = np.sqrt(X * X + Y * Y + Z * Z)
        v = (0.25 - np.abs(r - 0.6)).astype(np.float32)
        v[R // 2, R // 2, R // 2] = 1.0
    elif kind == "two_cubes":                                        # equal sizes: the lower label is the largest
        v, iso = np.zeros((R, R, R), np.float32), 0.5
        v[2:5, 3:6, 9:12] = 2.0
        v[10:13, 1:4, 2:5] = 3.0
        v[15, 15, 15] = 1.0
    else:
        raise KeyError(kind)
    v = np.ascontiguousarray(v, dtype=np.float32)
    v.setflags(write=False)
    ref = CC.components(v, iso)
    for a in ref:
        a.setflags(write=False)
    return v, iso, ref


# ------------------------------------------------------------------------------------------------ the C calls, poisoned
def _label_sizes(vol, iso, pattern):
    """nerf_ccl_label + nerf_ccl_sizes into sentinel outputs with one spare element, the workspace poisoned."""
    from nerf_meets_mlx_amd import _native as N
    L = N.lib()
    R = vol.shape[0]
    n3 = R ** 3
    ws = poison_(torch.empty(L.nerf_ccl_workspace_bytes(R), dtype=torch.uint8, device=DEV), pattern)
    labels = torch.full((n3 + 1,), SENT32, dtype=torch.int32, device=DEV)
    sizes = torch.full((n3 + 1,), SENT32, dtype=torch.int32, device=DEV)
    stats = torch.full((4,), SENT64, dtype=torch.int64, device=DEV)
    N.check(L.nerf_ccl_label(N.ptr(vol), R, float(iso), N.ptr(ws), N.ptr(labels), N.stream()))
    N.check(L.nerf_ccl_sizes(N.ptr(labels), R, N.ptr(sizes), N.ptr(stats), N.stream()))
    torch.cuda.synchronize()
    assert int(labels[n3]) == SENT32 and int(sizes[n3]) == SENT32 and int(stats[3]) == SENT64
    return labels[:n3], sizes[:n3], stats[:3]


def _filter(vol, comps, iso, min_voxels, largest_only, alias=False):
    from nerf_meets_mlx_amd import _native as N
    from tests._poison import sentinel_, unwritten
    R = vol.shape[0]
    n3 = R ** 3
    labels, sizes, stats = (t.contiguous() for t in comps)
    if alias:
        out = torch.cat([vol.reshape(-1), sentinel_(torch.empty(1, dtype=torch.float32, device=DEV))])
        src = out
    else:
        out = sentinel_(torch.empty(n3 + 1, dtype=torch.float32, device=DEV))
        src = vol
    N.check(N.lib().nerf_ccl_filter(N.ptr(src), N.ptr(labels), N.ptr(sizes), N.ptr(stats), R, float(iso), int(min_voxels),
                                    int(largest_only), N.ptr(out), N.stream()))
    torch.cuda.synchronize()
    assert unwritten(out[n3:]) == 1
    return out[:n3].view(R, R, R)


def _check_components(kind, R):
    v, iso, (wl, ws, wst) = _case(kind, R)
    vol = torch.from_numpy(v.copy()).to(DEV)
    got = None
    for pattern in PATTERNS:
        got = _label_sizes(vol, iso, pattern)
        assert torch.equal(got[0].cpu(), torch.from_numpy(wl.copy())), (kind, R, pattern)
        assert torch.equal(got[1].cpu(), torch.from_numpy(ws.copy())), (kind, R, pattern)
        assert got[2].tolist() == wst.tolist(), (kind, R, pattern)
    from nerf_meets_mlx_amd.engine import mesh
    c = mesh.connected_components(vol, iso)
    assert c.labels.shape == (R, R, R) and c.sizes.shape == (R, R, R) and c.labels.dtype == torch.int32
    assert torch.equal(c.labels.reshape(-1), got[0]) and torch.equal(c.sizes.reshape(-1), got[1]) and torch.equal(c.stats, got[2])
    return vol, iso, got, c


def _check_filter(kind, R, vol, iso, got, c, min_voxels, largest_only):
    from nerf_meets_mlx_amd.engine import mesh
    v, _, ref = _case(kind, R)
    want = torch.from_numpy(CC.filter_volume(v, iso, min_voxels, largest_only, comps=ref))
    out = _filter(vol, got, iso, min_voxels, largest_only)
    assert bits_equal(out.cpu(), want), (kind, R, min_voxels, largest_only)
    before = vol.clone()
    pub = mesh.filter_components(vol, iso, int(min_voxels), bool(largest_only), components=c)
    assert bits_equal(pub, out) and bits_equal(vol, before) and pub.data_ptr() != vol.data_ptr()
    return out


# ------------------------------------------------------------------------------------------------ labels, sizes, stats
@pytest.mark.parametrize("R", SIZES)
@pytest.mark.parametrize("kind", ["noise", "noise75", "checkerboard", "special", "all_inside", "all_outside"])
def test_components_match_the_reference_bit_for_bit(kind, R):
    vol, iso, got, c = _check_components(kind, R)
    n3 = R ** 3
    if kind == "all_inside":
        assert got[2].tolist() == [1, n3, 0] and int(got[1][0]) == n3 and bool((got[0] == 0).all())
    if kind == "all_outside":
        assert got[2].tolist() == [0, 0, -1] and bool((got[0] == -1).all()) and bool((got[1] == 0).all())
    if kind == "checkerboard":
        assert got[2].tolist()[:2] == [(n3 + 1) // 2, (n3 + 1) // 2]
    if kind == "noise" and R >= 64:                                  # above the percolation threshold: one giant component
        assert int(got[1].max()) > n3 // 4 and int(got[2][0]) > 1000
    if kind == "noise75" and R >= 64:                                # below it: no giant
        assert int(got[1].max()) < n3 // 50 and int(got[2][0]) > 1000


@pytest.mark.parametrize("kind,R", [("serpentine", 3), ("serpentine", 17), ("row_ends", 3), ("row_ends", 17),
                                    ("row_end_pairs", 3), ("row_end_pairs", 17), ("shell", 17), ("two_cubes", 17)])
def test_constructed_volumes(kind, R):
    vol, iso, got, c = _check_components(kind, R)
    st = got[2].tolist()
    if kind == "serpentine":
        assert st[0] == 1 and st[2] == 0 and st[1] >= (R ** 3) // 4
    if kind == "row_ends":
        assert st == [2, 2 * R * R, 0]
    if kind == "row_end_pairs":
        assert st[0] == st[1] > 0                                    # every voxel on its own
    if kind == "shell":
        assert st[0] == 2
        out = _check_filter(kind, R, vol, iso, got, c, 0, True)
        kept = out > iso
        assert int(kept.sum()) == st[1] - 1 and not bool(kept[R // 2, R // 2, R // 2])       # whole, the speck gone
    if kind == "two_cubes":
        first = 9 + R * (3 + R * 2)
        assert st == [3, 55, first]
        out = _check_filter(kind, R, vol, iso, got, c, 0, True)
        assert bool((out[2:5, 3:6, 9:12] == 2.0).all()) and int((out > iso).sum()) == 27
        _check_filter(kind, R, vol, iso, got, c, 27, False)
        _check_filter(kind, R, vol, iso, got, c, 28, True)


# ------------------------------------------------------------------------------------------------ filter
@pytest.mark.parametrize("R", [17, 65])
@pytest.mark.parametrize("kind", ["noise", "noise75", "special"])
def test_filter_matches_the_reference_bit_for_bit(kind, R):
    vol, iso, got, c = _check_components(kind, R)
    v, _, (wl, ws, wst) = _case(kind, R)
    root_sizes = np.sort(ws[ws > 0])
    largest = int(root_sizes[-1])
    for m in (0, 1, 2, int(np.median(root_sizes)), max(2, int(np.median(root_sizes[root_sizes > 1]))), largest, largest + 1):
        for only in (False, True):
            out = _check_filter(kind, R, vol, iso, got, c, m, only)
            if m <= 1 and not only:
                assert bits_equal(out, vol)
            if m == largest + 1:
                assert not bool((out > iso).any())
    # out may alias vol
    want = torch.from_numpy(CC.filter_volume(v, iso, 2, True, comps=(wl, ws, wst)))
    assert bits_equal(_filter(vol.clone(), got, iso, 2, True, alias=True).cpu(), want)
    if kind == "special":                                            # NaN payloads survive
        nan = np.isnan(v)
        assert torch.equal(_filter(vol, got, iso, 2, False).cpu().view(torch.int32)[torch.from_numpy(nan)],
                           torch.from_numpy(v.view(np.int32)[nan]))


def test_two_runs_are_bit_identical():
    from nerf_meets_mlx_amd.engine import mesh
    v, iso, _ = _case("noise", 65)
    vol = torch.from_numpy(v.copy()).to(DEV)
    a, b = mesh.connected_components(vol, iso), mesh.connected_components(vol, iso)
    assert torch.equal(a.labels, b.labels) and torch.equal(a.sizes, b.sizes) and torch.equal(a.stats, b.stats)
    assert bits_equal(mesh.filter_components(vol, iso, 5, True), mesh.filter_components(vol, iso, 5, True, components=a))


# ------------------------------------------------------------------------------------------------ through marching cubes
def test_filtered_volume_through_marching_cubes():
    from nerf_meets_mlx_amd.engine import mesh
    R, iso, lo, hi = 64, 0.0, [-1.1, -0.7, 0.3], [0.9, 1.6, 2.05]
    rng = np.random.default_rng(7)
    Z, Y, X = _centres(R)
    big = 0.5 - np.sqrt((X + 0.2) ** 2 + 1.4 * Y * Y + 0.7 * Z * Z)
    small = 0.15 - np.sqrt((X - 0.7) ** 2 + (Y - 0.6) ** 2 + (Z + 0.5) ** 2)
    v = np.maximum(big, small)
    specks = (rng.random((R, R, R)) < 0.004) & (v < -0.15)
    specks[[0, -1]] = specks[:, [0, -1]] = specks[:, :, [0, -1]] = False
    v = np.where(specks, 0.3, v).astype(np.float32)
    comps = CC.components(v, iso)
    assert comps[2][0] > 50
    vol = torch.from_numpy(v).to(DEV)
    m = mesh.marching_cubes(mesh.filter_components(vol, iso, largest_only=True), iso, lo, hi)
    wv, wf, wn = M.marching_cubes(CC.filter_volume(v, iso, 0, True, comps=comps), iso, lo, hi)
    assert bits_equal(m.verts.cpu(), torch.from_numpy(wv)) and torch.equal(m.faces.cpu(), torch.from_numpy(wf))
    assert float((m.normals.cpu() - torch.from_numpy(wn)).abs().max()) <= 1e-6
    assert M.closed_and_oriented(wf) and M.euler(wv, wf) == 2
    full = mesh.marching_cubes(vol, iso, lo, hi)
    keep = torch.from_numpy(CC.kept_vertex_mask(v, iso, CC.dropped_mask(*comps, 0, True)))
    assert 0 < int(keep.sum()) < full.verts.shape[0] == keep.shape[0]
    assert bits_equal(full.verts.cpu()[keep], m.verts.cpu())


# ------------------------------------------------------------------------------------------------ trainer
def test_march_trainer_extract_mesh_with_the_filter(tmp_path):
    """test_gpu_mesh.py's march-mode fixture (hw 48, 2^14-entry tables), a handful of iterations, R = 32."""
    from nerf_meets_mlx_amd.dataset import synthetic
    from nerf_meets_mlx_amd.engine import mesh
    from nerf_meets_mlx_amd.engine.ngp import NGPTrainer
    imgs, poses, _, _, K = synthetic.make_dataset(48, 48, 8, seed=0, device=DEV)
    tr = NGPTrainer(imgs, poses, K, N_rand=256, n_depth_samples=64, seed=4, device=DEV, log2_hashmap_size=14,
                    occupancy_grid=True, march_steps=1024)
    for _ in range(20):
        tr.train_step()
    R, lo, hi = 32, [-1.5] * 3, [1.5] * 3
    vol = tr.density_volume(R)
    thr = float(vol.reshape(-1).quantile(0.9))
    assert float(vol.min()) < thr < float(vol.max())
    query, act = tr._mesh_field()
    # defaults: today's call, bit for bit
    a = tr.extract_mesh(R, threshold=thr)
    b = mesh.extract(query, act, R, thr, lo, hi, colors=True, device=tr.device)
    assert bits_equal(a.verts, b.verts) and torch.equal(a.faces, b.faces) and bits_equal(a.normals, b.normals)
    assert bits_equal(a.colors, b.colors)
    wv, wf, _ = M.marching_cubes(vol.cpu().numpy(), thr, lo, hi)
    assert bits_equal(a.verts.cpu(), torch.from_numpy(wv)) and torch.equal(a.faces.cpu(), torch.from_numpy(wf))
    # filtered: density_volume -> filter_components -> marching cubes (+ colours) by hand
    c = mesh.connected_components(vol, thr)
    assert int(c.stats[0]) >= 1
    got = tr.extract_mesh(R, threshold=thr, min_component=2, largest_only=True)
    f = mesh.filter_components(vol, thr, 2, True, components=c)
    want, rows = mesh._marching_cubes(f, thr, lo, hi, True)
    assert bits_equal(got.verts, want.verts) and torch.equal(got.faces, want.faces) and bits_equal(got.normals, want.normals)
    assert bits_equal(got.colors, mesh.vertex_colors(query, rows))
    assert bits_equal(f.cpu(), torch.from_numpy(CC.filter_volume(vol.cpu().numpy(), thr, 2, True)))
    assert got.verts.shape[0] <= a.verts.shape[0]
    plain = tr.extract_mesh(R, threshold=thr, colors=False, min_component=2, largest_only=True)
    assert plain.colors is None and bits_equal(plain.verts, got.verts) and torch.equal(plain.faces, got.faces)
    back = mesh.read_ply(mesh.write_ply(str(tmp_path / "filtered.ply"), got))
    assert bits_equal(back.verts, got.verts.cpu()) and torch.equal(back.faces, got.faces.cpu())
    assert back.verts.shape[0] == got.verts.shape[0] and back.faces.shape[0] == got.faces.shape[0]
