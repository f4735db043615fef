"""Morphological opening on the GPU (csrc/morph.hip, engine/mesh/volume.py erode / reconstruct / open_components, extract_mesh's
opening_radius) against the reference of tests/_morph_ref.py: eroded and reconstructed volumes and their stats bit for bit, into
sentinel outputs with one spare element and a poisoned workspace, at lattice sizes around the 64-voxel mask word (word tails,
exactly one word, one word + 1), at radii up to the largest (r >= R / 2: an empty core, everything dropped), on the volumes a
bit-packed step goes wrong on; aliasing; reproducibility; the pipeline through marching cubes; a march-mode trainer's opened
mesh through write_ply."""
import functools

import numpy as np
import pytest
import torch

from tests import _ccl_ref as CC
from tests import _mesh_ref as M
from tests import _morph_ref as MR
from tests._poison import PATTERNS, bits_equal, poison_, sentinel_, unwritten

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT64 = 0x7FE5A5A57FE5A5A5
SIZES = [2, 3, 17, 31, 32, 33, 64, 65]
RADII = [1, 2, 3, 16]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"


# ------------------------------------------------------------------------------------------------ volumes
@functools.lru_cache(maxsize=None)
def _case(kind, R):
    """(volume float32 [R, R, R], iso) -- computed once per module run, never changed."""
    rng = np.random.default_rng(200 + R)
    iso = 0.0
    if kind in ("noise40", "noise70"):
        v = MR.smoothed_noise(R, 300 + R)
        iso = float(np.quantile(v, 0.4 if kind == "noise40" else 0.7))
    elif kind == "all_inside":
        v, iso = np.full((R, R, R), 2.0, np.float32), 1.0
    elif kind == "all_outside":
        v, iso = np.full((R, R, R), 2.0, np.float32), 2.0            # v == iso is outside
    elif kind == "special":                                          # NaN, +-inf and exact-iso voxels in a thick blob
        x = (np.arange(R) + 0.5) / R * 2 - 1
        Z, Y, X = np.meshgrid(x, x, x, indexing="ij")
        v = (0.9 - np.sqrt(X * X + 1.3 * Y * Y + 0.8 * Z * Z) + 0.05 * rng.standard_normal((R, R, R))).astype(np.float32)
        flat = v.reshape(-1)
        idx = rng.permutation(flat.size)
        n = max(1, flat.size // 40)
        flat[idx[:n]] = np.nan
        flat[idx[n:2 * n]] = np.inf
        flat[idx[2 * n:3 * n]] = -np.inf
        flat[idx[3 * n:4 * n]] = 0.0
        flat.view(np.uint32)[idx[:n:2]] = 0x7FC12345                 # NaNs with a payload
    elif kind == "row_ends":                                         # sheets 2 thick at i = 0, 1 and i = R - 2, R - 1, full in y, z:
        v, iso = np.zeros((R, R, R), np.float32), 0.5                # across a row end they would look 4 thick and keep a core
        v[:, :, :min(2, R)] = 1.0
        v[:, :, max(0, R - 2):] = 2.0
    elif kind == "word_block":                                       # a solid block across every 64-voxel word boundary of a row
        v, iso = np.zeros((R, R, R), np.float32), 0.5
        b = R // 2 if R <= 32 else 32 if R <= 64 else 64            # R <= 32: one word, the block sits mid-row
        a0, a1 = max(0, b - 5), min(R, b + 5)
        v[:, :, a0:a1] = 1.0 + rng.random((R, R, a1 - a0)).astype(np.float32)
    else:
        raise KeyError(kind)
    v = np.ascontiguousarray(v, dtype=np.float32)
    v.setflags(write=False)
    return v, iso


# ------------------------------------------------------------------------------------------------ the C calls, poisoned
def _dev(a):
    return torch.from_numpy(np.array(a, copy=True)).to(DEV)


def _call(which, vol, kept, iso, r, pattern, alias=None):
    """nerf_morph_erode / nerf_morph_reconstruct into a sentinel output with one spare element (or, with alias = "vol" / "kept",
    into a copy of that input with a spare element), stats with a spare word, the workspace poisoned."""
    from nerf_meets_mlx_amd import _native as N
    L = N.lib()
    R = vol.shape[0]
    n3 = R ** 3
    ws = poison_(torch.empty(L.nerf_morph_workspace_bytes(R), dtype=torch.uint8, device=DEV), pattern)
    spare = sentinel_(torch.empty(1, dtype=torch.float32, device=DEV))
    out = sentinel_(torch.empty(n3 + 1, dtype=torch.float32, device=DEV))
    if alias == "vol":
        vol = out = torch.cat([vol.reshape(-1), spare])
    elif alias == "kept":
        kept = out = torch.cat([kept.reshape(-1), spare])
    stats = torch.full((3,), SENT64, dtype=torch.int64, device=DEV)
    if which == "erode":
        N.check(L.nerf_morph_erode(N.ptr(vol), R, float(iso), int(r), N.ptr(ws), N.ptr(out), N.ptr(stats), N.stream()))
    else:
        N.check(L.nerf_morph_reconstruct(N.ptr(vol), N.ptr(kept), R, float(iso), int(r), N.ptr(ws), N.ptr(out), N.ptr(stats),
                                         N.stream()))
    torch.cuda.synchronize()
    assert unwritten(out[n3:]) == 1 and int(stats[2]) == SENT64
    return out[:n3].view(R, R, R), stats[:2]


def _check_erode(v, iso, r, tag):
    want, wst = MR.erode(v, iso, r)
    vol = _dev(v)
    for pattern in PATTERNS:
        got, st = _call("erode", vol, None, iso, r, pattern)
        assert bits_equal(got.cpu(), torch.from_numpy(want)), (tag, r, pattern)
        assert st.tolist() == wst.tolist(), (tag, r, pattern)
    assert bits_equal(vol.cpu(), torch.from_numpy(np.array(v)))       # the input is left alone
    return want, wst


def _check_reconstruct(v, kept, iso, r, tag):
    want, wst = MR.reconstruct(v, kept, iso, r)
    vol, k = _dev(v), _dev(kept)
    for pattern in PATTERNS:
        got, st = _call("reconstruct", vol, k, iso, r, pattern)
        assert bits_equal(got.cpu(), torch.from_numpy(want)), (tag, r, pattern)
        assert st.tolist() == wst.tolist(), (tag, r, pattern)
    return want, wst


def _seeds(v, iso, R, seed):
    """A volume whose inside set is random and lies partly outside {v > iso}; other values on both sides of iso, NaN among them."""
    rng = np.random.default_rng(seed)
    k = np.where(rng.random((R, R, R)) < 0.02, np.float32(iso + 1.0), np.float32(iso - 1.0)).astype(np.float32)
    k.reshape(-1)[::7] = iso
    k.reshape(-1)[3::31] = np.nan
    return k


# ------------------------------------------------------------------------------------------------ erode, reconstruct
@pytest.mark.parametrize("R", SIZES)
@pytest.mark.parametrize("kind", ["noise40", "noise70", "all_inside", "all_outside", "special", "row_ends", "word_block"])
def test_erode_and_reconstruct_match_the_reference_bit_for_bit(kind, R):
    v, iso = _case(kind, R)
    m = CC.inside_mask(v, iso)
    face = np.minimum(np.arange(R), R - 1 - np.arange(R))
    for r in RADII:
        core, est = _check_erode(v, iso, r, (kind, R))
        out, rst = _check_reconstruct(v, core, iso, r, (kind, R))     # K = E: the opening by reconstruction
        assert est.tolist()[1] == rst.tolist()[0] <= rst.tolist()[1] <= est.tolist()[0] == int(m.sum())
        if kind == "all_inside":                                     # the voxels >= r from every face; back: all but what an
            n = max(0, R - 2 * r)                                    # L1 ball cannot reach (the box's edges and corners)
            short = np.maximum(0, r - face)
            back = (short[:, None, None] + short[None, :, None] + short[None, None, :] <= r) & (n > 0)
            assert est.tolist() == [R ** 3, n ** 3] and np.array_equal(CC.inside_mask(out, iso), back)
        if kind == "all_outside":
            assert est.tolist() == [0, 0] and rst.tolist() == [0, 0] and np.array_equal(out.view(np.uint32), v.view(np.uint32))
        if kind == "row_ends" and R >= 5:                            # 2 thick: no core, whatever lies past the row's end
            assert est.tolist() == [int(m.sum()), 0] and not CC.inside_mask(out, iso).any()
        if 2 * r >= R:                                               # r >= R / 2: an empty core, everything is dropped
            assert est.tolist()[1] == 0 and not CC.inside_mask(out, iso).any()
        if kind == "special":                                        # NaN payloads survive both calls
            nan = np.isnan(v)
            assert np.array_equal(core.view(np.uint32)[nan], v.view(np.uint32)[nan])
            assert np.array_equal(out.view(np.uint32)[nan], v.view(np.uint32)[nan])
    # seeds partly outside M, and no seeds at all
    for r in (1, 3):
        k = _seeds(v, iso, R, 7 + R)
        _, st = _check_reconstruct(v, k, iso, r, (kind, R, "seeds"))
        assert st.tolist()[0] == int((CC.inside_mask(k, iso) & m).sum())
        want, st = _check_reconstruct(v, np.full((R, R, R), iso, np.float32), iso, r, (kind, R, "no seeds"))
        assert st.tolist() == [0, 0] and not CC.inside_mask(want, iso).any()


def test_sheets_at_the_two_row_ends_do_not_support_each_other():
    """One voxel at i = R - 1 of row j and one at i = 0 of row j + 1 are adjacent in memory (and, at R = 64, bit 63 of one mask
    word and bit 0 of the next): a seed in one must not reach the other, and neither is the other's neighbour in the erosion."""
    for R in (3, 17, 64, 65):
        v = np.zeros((R, R, R), np.float32)
        v[:, :, R - 1] = 1.0
        v[:, :, 0] = 2.0
        kept = np.zeros_like(v)
        kept[:, :, R - 1] = 1.0                                      # seeds: the sheet at i = R - 1 only
        for r in (1, 2):
            out, st = _check_reconstruct(v, kept, 0.5, r, ("sheets", R))
            assert st.tolist() == [R * R, R * R] and not (out[:, :, 0] > 0.5).any() and (out[:, :, R - 1] > 0.5).all()
            _, est = _check_erode(v, 0.5, r, ("sheets", R))
            assert est.tolist() == [2 * R * R, 0]
        # a slab 3 thick at each row end has a core 1 thick only if the lattice's faces did not erode: they do
        w = np.zeros((R, R, R), np.float32)
        w[:, :, :min(3, R)] = 1.0
        w[:, :, max(0, R - 3):] = 1.0
        if R >= 6:
            _, est = _check_erode(w, 0.5, 1, ("slabs", R))
            assert est.tolist() == [6 * R * R, 2 * (R - 2) ** 2]


@pytest.mark.parametrize("R,big,small,length", [(17, 7, 5, 5), (33, 13, 9, 11), (65, 31, 9, 25)])
def test_dumbbells(R, big, small, length):
    iso = 0.5
    for width in (1, 2):
        for at in (0, 2):
            v, bridge, cube = MR.dumbbell(R, big, small, width, length, at)
            for r in (1, 2):
                core, est = _check_erode(v, iso, r, ("dumbbell", R, width, at))
                comps = CC.components(core, iso)
                assert not (CC.inside_mask(core, iso) & bridge).any()     # 2 wide at most: the bar has no core
                assert comps[2].tolist()[0] == (2 if small > 2 * r else 1)
                kept = CC.filter_volume(core, iso, 0, True, comps=comps)
                out, _ = _check_reconstruct(v, kept, iso, r, ("dumbbell", R, width, at))
                d = CC.inside_mask(out, iso)
                assert not (d & ~cube & ~bridge).any() and int((d & bridge).sum()) <= r * width * width
    v, bridge, _ = MR.dumbbell()
    assert int(bridge.sum()) == 5 and _check_erode(v, iso, 1, "dumbbell")[1].tolist() == [473, 152]


@pytest.mark.parametrize("R", [17, 65])
def test_reconstruction_does_not_jump_a_gap(R):
    iso = 0.5
    for gap in (1, 2):
        v, seeds, upper = MR.c_channel(R, gap)
        m = CC.inside_mask(v, iso)
        kept = np.where(seeds, v, np.float32(0.0)).astype(np.float32)
        for r in (2, 3):
            out, _ = _check_reconstruct(v, kept, iso, r, ("c", R, gap))
            d = CC.inside_mask(out, iso)
            assert not (d & upper).any() and (seeds <= d).all()
            if gap < r:
                assert (MR.dilate_ball(seeds, r) & m & upper).any()  # plain dilate-and-mask would reach the other arm


@pytest.mark.parametrize("R", [17, 65])
def test_outputs_may_alias_inputs(R):
    v, iso = _case("noise40", R)
    for r in (1, 3):
        core, wst = MR.erode(v, iso, r)
        got, st = _call("erode", _dev(v), None, iso, r, PATTERNS[0], alias="vol")
        assert bits_equal(got.cpu(), torch.from_numpy(core)) and st.tolist() == wst.tolist()
        kept = CC.filter_volume(core, iso, 0, True)
        want, wst = MR.reconstruct(v, kept, iso, r)
        for alias in ("vol", "kept"):
            got, st = _call("reconstruct", _dev(v), _dev(kept), iso, r, PATTERNS[1], alias=alias)
            assert bits_equal(got.cpu(), torch.from_numpy(want)) and st.tolist() == wst.tolist(), alias


def test_two_runs_are_bit_identical():
    from nerf_meets_mlx_amd.engine import mesh
    v, iso = _case("noise40", 65)
    vol = _dev(v)
    (a, sa), (b, sb) = mesh.erode(vol, iso, 2), mesh.erode(vol, iso, 2)
    assert bits_equal(a, b) and torch.equal(sa, sb) and a.data_ptr() != vol.data_ptr()
    (c, sc), (d, sd) = mesh.reconstruct(vol, a, iso, 2), mesh.reconstruct(vol, b, iso, 2)
    assert bits_equal(c, d) and torch.equal(sc, sd) and sa.device.type == "cuda" and sc.dtype == torch.int64
    assert bits_equal(mesh.open_components(vol, iso, 2, 5, True), mesh.open_components(vol, iso, 2, 5, True))


# ------------------------------------------------------------------------------------------------ the pipeline
@pytest.mark.parametrize("kind,R", [("noise40", 17), ("noise40", 33), ("noise70", 65), ("special", 64)])
def test_open_components_matches_the_reference_pipeline(kind, R):
    from nerf_meets_mlx_amd.engine import mesh
    v, iso = _case(kind, R)
    vol = _dev(v)
    before = vol.clone()
    for r in (1, 2):
        core, stats = mesh.erode(vol, iso, r)
        wcore, wst = MR.erode(v, iso, r)
        assert bits_equal(core.cpu(), torch.from_numpy(wcore)) and stats.tolist() == wst.tolist()
        c = mesh.connected_components(core, iso)                     # the GPU's labels (tested against _ccl_ref on their own)
        comps = (c.labels.cpu().numpy().reshape(-1), c.sizes.cpu().numpy().reshape(-1), c.stats.cpu().numpy())
        for kw in (dict(), dict(largest_only=True), dict(min_component=2), dict(min_component=30, largest_only=True)):
            got = mesh.open_components(vol, iso, r, **kw)
            want = MR.open_components(v, iso, r, comps=comps, **kw)
            assert bits_equal(got.cpu(), torch.from_numpy(want)), (kind, R, r, kw)
            assert got.data_ptr() != vol.data_ptr()
        out, rst = mesh.reconstruct(vol, core, iso, r)
        assert bits_equal(out, mesh.open_components(vol, iso, r)) and int(rst[0]) == int(stats[1])
    assert bits_equal(vol, before)


def _field_of(v):
    """A query whose density volume over [-1, 1]^3 is `v` (>= 0) bit for bit: raw[..., 3] = v at the lattice point nearest to the
    row's origin, and a colour that depends on the position."""
    R = v.shape[0]
    flat = v.reshape(-1)

    def query(rows, z):
        idx = ((rows[:, :3] + 1.0) * (R / 2.0) - 0.5).round().long().clamp(0, R - 1)      # the lattice point nearest to o
        sig = flat[idx[:, 0] + R * (idx[:, 1] + R * idx[:, 2])]
        rgb = (rows[:, :3] * 0.5 + 0.5).clamp(0, 1)
        return torch.cat([rgb, sig[:, None]], 1).reshape(-1, 1, 4)
    return query


def test_extract_with_and_without_the_opening_through_marching_cubes():
    from nerf_meets_mlx_amd.engine import mesh
    R, iso, lo, hi, r = 19, 0.5, [-1.0] * 3, [1.0] * 3, 1
    v, bridge, cube = MR.dumbbell(R, x0=1)                           # clear of the box's faces: the meshes are closed
    rng = np.random.default_rng(3)
    v = np.where(v > iso, v + rng.random(v.shape).astype(np.float32), np.float32(0.1) * rng.random(v.shape).astype(np.float32))
    v = np.ascontiguousarray(v, dtype=np.float32)
    vol = _dev(v)
    query = _field_of(vol)
    assert bits_equal(mesh.density_volume(query, mesh.RELU, R, lo, hi, device=DEV), vol)
    # opening_radius = 0: today's call, bit for bit, with and without min_component
    for kw in (dict(), dict(min_component=3), dict(largest_only=True)):
        a = mesh.extract(query, mesh.RELU, R, iso, lo, hi, colors=True, device=DEV, opening_radius=0, **kw)
        f = mesh.filter_components(vol, iso, **kw) if kw else vol
        b, rows = mesh._marching_cubes(f, iso, lo, hi, True)
        assert bits_equal(a.verts, b.verts) and torch.equal(a.faces, b.faces) and bits_equal(a.normals, b.normals)
        assert bits_equal(a.colors, mesh.vertex_colors(query, rows))
    # the filter alone keeps the whole dumbbell (one component); the opening cuts the bridge and the small cube goes
    full = mesh.marching_cubes(vol, iso, lo, hi)
    only = mesh.extract(query, mesh.RELU, R, iso, lo, hi, colors=False, device=DEV, largest_only=True)
    assert bits_equal(only.verts, full.verts)
    got = mesh.extract(query, mesh.RELU, R, iso, lo, hi, colors=False, device=DEV, largest_only=True, opening_radius=r)
    wvol = MR.open_components(v, iso, r, 0, True)
    d = CC.inside_mask(wvol, iso)
    assert d.any() and not (d & ~cube).any()
    wv, wf, wn = M.marching_cubes(wvol, iso, lo, hi)
    assert bits_equal(got.verts.cpu(), torch.from_numpy(wv)) and torch.equal(got.faces.cpu(), torch.from_numpy(wf))
    assert float((got.normals.cpu() - torch.from_numpy(wn)).abs().max()) <= 1e-6
    assert M.closed_and_oriented(wf) and M.euler(wv, wf) == 2
    in_out, in_vol = MR.original_edge_masks(v, wvol, iso)
    assert 0 < int(in_out.sum()) < len(in_out) == got.verts.shape[0] and len(in_vol) == full.verts.shape[0]
    assert bits_equal(got.verts.cpu()[torch.from_numpy(in_out)], full.verts.cpu()[torch.from_numpy(in_vol)])


# ------------------------------------------------------------------------------------------------ trainer
def test_march_trainer_extract_mesh_with_the_opening(tmp_path):
    """test_gpu_ccl.py's march-mode fixture (hw 48, 2^14-entry tables), a handful of iterations, R = 32."""
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
    thr = float(vol.reshape(-1).quantile(0.7))
    assert float(vol.min()) < thr < float(vol.max())
    query, act = tr._mesh_field()
    # opening_radius = 0: today's call
    a = tr.extract_mesh(R, threshold=thr, min_component=2, largest_only=True)
    b = tr.extract_mesh(R, threshold=thr, min_component=2, largest_only=True, opening_radius=0)
    assert bits_equal(a.verts, b.verts) and torch.equal(a.faces, b.faces) and bits_equal(a.colors, b.colors)
    # opened: density_volume -> open_components -> marching cubes (+ colours) by hand, and the reference's volume
    got = tr.extract_mesh(R, threshold=thr, min_component=2, largest_only=True, opening_radius=1)
    f = mesh.open_components(vol, thr, 1, 2, True)
    want, rows = mesh._marching_cubes(f, thr, lo, hi, True)
    assert bits_equal(got.verts, want.verts) and torch.equal(got.faces, want.faces) and bits_equal(got.normals, want.normals)
    assert bits_equal(got.colors, mesh.vertex_colors(query, rows))
    assert bits_equal(f.cpu(), torch.from_numpy(MR.open_components(vol.cpu().numpy(), thr, 1, 2, True)))
    assert int((f > thr).sum()) <= int((vol > thr).sum())
    plain = tr.extract_mesh(R, threshold=thr, colors=False, min_component=2, largest_only=True, opening_radius=1)
    assert plain.colors is None and bits_equal(plain.verts, got.verts) and torch.equal(plain.faces, got.faces)
    back = mesh.read_ply(mesh.write_ply(str(tmp_path / "opened.ply"), got))
    assert bits_equal(back.verts, got.verts.cpu()) and torch.equal(back.faces, got.faces.cpu())
    assert back.verts.shape[0] == got.verts.shape[0] and back.faces.shape[0] == got.faces.shape[0]
