"""Mesh simplification on the GPU (csrc/simplify.hip, engine/mesh/surface.py simplify, Trainer.extract_mesh / NGPTrainer.extract_mesh_tsdf
with simplify_grid) against the numpy reference of tests/_simplify_ref.py: vertex, normal and colour bits compared as integers and
faces exactly -- no tolerance anywhere, the rule is exact -- into sentinel-filled outputs with a poisoned workspace;
reproducibility under a permutation of the input; empty meshes and total collapse; long runs of faces on one vertex set; the C
ABI's argument errors; a march-mode trainer's simplified mesh through write_ply."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _simplify_ref as S
from tests._poison import NAN_BYTES, PATTERNS, bits_equal, poison_, sentinel_, unwritten

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT32 = 0x7FE5A5A5
E_NULL, E_SHAPE = -1, -2


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"


def _dev(a, dtype):
    return torch.from_numpy(np.array(a, order="C")).to(device=DEV, dtype=dtype).contiguous()


def _simplify_poisoned(v, f, n, c, G, placement, pattern=NAN_BYTES, lo=S.LO, hi=S.HI):
    """The C calls of engine.mesh.simplify on numpy inputs, with a poisoned workspace and sentinel outputs that carry one spare
    row each; (verts, faces, normals, colors or None, rows) as numpy arrays, K."""
    from nerf_meets_mlx_amd import _native as N
    L = N.lib()
    tv, tn, tf = _dev(v, torch.float32).reshape(-1, 3), _dev(n, torch.float32).reshape(-1, 3), _dev(f, torch.int32).reshape(-1, 3)
    tc = None if c is None else _dev(c, torch.float32).reshape(-1, 3)
    V, F = tv.shape[0], tf.shape[0]
    clo, chi = (C.c_float * 3)(*lo), (C.c_float * 3)(*hi)
    nbytes = L.nerf_simplify_workspace_bytes(V, F, G)
    assert nbytes > 0
    ws = poison_(torch.empty(nbytes, dtype=torch.uint8, device=DEV), pattern)
    keys = torch.full((F,), -7, dtype=torch.int64, device=DEV)
    tot = torch.full((3,), -7, dtype=torch.int64, device=DEV)
    N.check(L.nerf_simplify_cluster(N.ptr(tv), N.ptr(tn), N.ptr(tc), V, N.ptr(tf), F, clo, chi, G, N.ptr(ws), N.ptr(keys), N.stream()))
    skeys, perm = torch.sort(keys, stable=True)
    N.check(L.nerf_simplify_count(N.ptr(skeys), N.ptr(perm), V, N.ptr(tf), F, G, N.ptr(ws), N.ptr(tot), N.stream()))
    V2, F2, K = tot.tolist()
    ov = sentinel_(torch.empty(V2 + 1, 3, dtype=torch.float32, device=DEV))
    on = sentinel_(torch.empty(V2 + 1, 3, dtype=torch.float32, device=DEV))
    oc = None if c is None else sentinel_(torch.empty(V2 + 1, 3, dtype=torch.float32, device=DEV))
    rows = sentinel_(torch.empty(V2 + 1, 11, dtype=torch.float32, device=DEV))
    of = torch.full((F2 + 1, 3), SENT32, dtype=torch.int32, device=DEV)
    N.check(L.nerf_simplify_write(V, N.ptr(tf), F, clo, chi, G, S.PLACEMENTS[placement], N.ptr(ws), V2, F2, N.ptr(ov), N.ptr(on),
                                  N.ptr(oc), N.ptr(rows), N.ptr(of), N.stream()))
    torch.cuda.synchronize()
    assert unwritten(ov[V2:]) == 3 and unwritten(on[V2:]) == 3 and unwritten(rows[V2:]) == 11
    assert unwritten(ov[:V2]) == 0 and unwritten(on[:V2]) == 0 and unwritten(rows[:V2]) == 0
    assert oc is None or (unwritten(oc[V2:]) == 3 and unwritten(oc[:V2]) == 0)
    assert bool((of[F2:] == SENT32).all())
    if F:
        assert np.array_equal(keys.cpu().numpy()[perm.cpu().numpy()], skeys.cpu().numpy())
    out = (ov[:V2].cpu().numpy(), of[:F2].cpu().numpy(), on[:V2].cpu().numpy(), None if oc is None else oc[:V2].cpu().numpy(),
           rows[:V2].cpu().numpy())
    return out, K


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _assert_same(got, want, what=""):
    gv, gf, gn, gc, rows = got
    wv, wf, wn, wc = want
    assert gv.shape == wv.shape and gf.shape == wf.shape, (what, gv.shape, wv.shape, gf.shape, wf.shape)
    assert np.array_equal(gf, wf), what
    dv = _bits(gv) != _bits(wv)
    assert not dv.any(), (what, "vertex bits differ", int(dv.sum()), gv[dv.any(1)][:4], wv[dv.any(1)][:4])
    assert np.array_equal(_bits(gn), _bits(wn)), (what, "normal bits differ")
    assert (gc is None) == (wc is None)
    if wc is not None:
        assert np.array_equal(_bits(gc), _bits(wc)), (what, "colour bits differ")
    want_rows = np.zeros((len(wv), 11), np.float32)
    want_rows[:, 0:3], want_rows[:, 3:6], want_rows[:, 8:11] = wv, -wn, -wn
    assert np.array_equal(_bits(rows), _bits(want_rows)), (what, "colour rows differ")


# ------------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("G", S.GRIDS)
@pytest.mark.parametrize("name", ["sphere", "box", "plate", "noise"])
def test_simplify_matches_the_reference_bit_for_bit(name, G):
    v, f, n, c = S.mesh(name)
    for k, (placement, colors) in enumerate([("quadric", True), ("quadric", False), ("mean", True), ("mean", False)]):
        (want, info) = S.expected(name, G, placement, colors)
        got, K = _simplify_poisoned(v, f, n, c if colors else None, G, placement, PATTERNS[k % 2])
        assert K == info["K"]
        _assert_same(got, want, (name, G, placement, colors))


def test_special_values_invalid_vertices_and_indices():
    """NaN / inf coordinates, indices outside [0, V), non-finite normals, NaN and out-of-range colours, vertices outside the box."""
    v, f, n, c = (a.copy() for a in S.mesh("sphere"))
    v[7, 1], v[400, 0], v[900, 2] = np.nan, np.inf, -np.inf
    v[50] = [3.0, -2.5, 0.1]                                         # outside the box: clamped into the border cells
    v[51] = [-1.0, 1.0, 0.25]                                        # on the box faces and on a cell face
    f[10, 2], f[11, 0], f[12, 1], f[13, 1] = len(v), -1, np.iinfo(np.int32).max, np.iinfo(np.int32).min
    n[3], n[60, 0], n[61] = np.nan, np.inf, 0.0
    c[5, 0], c[6], c[8, 2] = np.nan, [np.inf, -np.inf, 2.0], -0.0
    for G in (8, 12):
        for placement in ("quadric", "mean"):
            want = S.simplify(v, f, n, c, G, S.LO, S.HI, placement)
            got, _ = _simplify_poisoned(v, f, n, c, G, placement)
            _assert_same(got, want, (G, placement))
    lo, hi = [-0.9, -1.1, -0.7], [1.3, 0.8, 1.0]                    # a box that is no cube and whose cells are no binary fractions
    want = S.simplify(v, f, n, c, 7, lo, hi, "quadric")
    got, _ = _simplify_poisoned(v, f, n, c, 7, "quadric", lo=lo, hi=hi)
    _assert_same(got, want, "odd box")


def test_large_grid_and_more_than_one_scan_block():
    """G = 160: 64 000 mask words (more than one workgroup of the word scan, G^3 no multiple of 64 x 256) and every vertex of
    the sphere in a cell of its own or nearly; G = 512: the largest mask."""
    v, f, n, c = S.mesh("sphere")
    for G in (160, 512):
        want = S.simplify(v, f, n, c, G, S.LO, S.HI, "quadric")
        got, _ = _simplify_poisoned(v, f, n, c, G, "quadric")
        _assert_same(got, want, G)


# ------------------------------------------------------------------------------------------------ reproducibility
def test_two_calls_and_a_permuted_input_give_the_same_bits():
    v, f, n, c = S.mesh("noise")
    a, _ = _simplify_poisoned(v, f, n, c, 8, "quadric", PATTERNS[0])
    b, _ = _simplify_poisoned(v, f, n, c, 8, "quadric", PATTERNS[1])
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))
    rng = np.random.default_rng(11)
    pv, pf = rng.permutation(len(v)), rng.permutation(len(f))
    inv = np.empty(len(v), np.int64)
    inv[pv] = np.arange(len(v))
    p, _ = _simplify_poisoned(v[pv], inv[f].astype(np.int32)[pf], n[pv], c[pv], 8, "quadric")
    for k in (0, 2, 3):
        assert np.array_equal(_bits(a[k]), _bits(p[k])), k
    assert np.array_equal(np.unique(a[1], axis=0, return_counts=True)[0], np.unique(p[1], axis=0, return_counts=True)[0])
    assert np.array_equal(np.unique(a[1], axis=0, return_counts=True)[1], np.unique(p[1], axis=0, return_counts=True)[1])


# ------------------------------------------------------------------------------------------------ empty and total collapse
def test_empty_inputs_and_total_collapse():
    from nerf_meets_mlx_amd.engine import mesh as E
    v, f, n, c = S.mesh("small")
    assert len(v) > 0 and len(f) > 0
    z3, zf = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    for vv, ff, nn, cc in ((z3, zf, z3, z3), (v, zf, n, c), (z3, zf, z3, None)):
        got, K = _simplify_poisoned(vv, ff, nn, cc, 4, "quadric")
        assert got[0].shape == (0, 3) and got[1].shape == (0, 3) and K == 0
    got, K = _simplify_poisoned(v, f, n, c, 2, "quadric")            # the whole sphere inside one cell
    assert K == 1 and got[0].shape == (0, 3) and got[1].shape == (0, 3)
    m = E.simplify(E.Mesh(_dev(v, torch.float32), _dev(f, torch.int32), _dev(n, torch.float32), _dev(c, torch.float32)), 2, S.LO, S.HI)
    assert m.verts.shape == (0, 3) and m.faces.shape == (0, 3) and m.normals.shape == (0, 3) and m.colors.shape == (0, 3)
    m = E.simplify(E.Mesh(_dev(z3, torch.float32), _dev(zf, torch.int32), _dev(z3, torch.float32)), 4, S.LO, S.HI, "mean")
    assert m.verts.shape == (0, 3) and m.faces.shape == (0, 3) and m.colors is None


# ------------------------------------------------------------------------------------------------ runs
@pytest.mark.parametrize("even,odd", [(50000, 0), (25000, 25000), (25001, 24999)])
def test_long_runs_on_one_vertex_set(even, odd):
    """Three vertices in three cells, 50 000 faces on them, the two orientations interleaved by a fixed shuffle."""
    v = np.array([[-0.5, -0.5, -0.5], [0.5, -0.5, -0.5], [-0.5, 0.5, 0.5]], np.float32)
    n = np.zeros((3, 3), np.float32)
    rots = np.array([[0, 1, 2], [1, 2, 0], [2, 0, 1]], np.int32)
    rng = np.random.default_rng(even)
    is_odd = rng.permutation(np.arange(even + odd) < odd)
    f = rots[rng.integers(0, 3, even + odd)]
    f[is_odd] = f[is_odd][:, ::-1]
    (gv, gf, gn, _, _), K = _simplify_poisoned(v, f, n, None, 2, "mean")
    assert K == 3
    keep = np.zeros(len(f), bool)
    if even != odd:
        keep[np.nonzero(~is_odd)[0][min(even, odd):]] = True
    assert len(gf) == keep.sum() == abs(even - odd)
    assert np.array_equal(gf, f[keep])
    if keep.any():
        assert np.array_equal(_bits(gv), _bits(v)) and not gn.any()
    else:
        assert gv.shape == (0, 3)
    want = S.simplify(v, f, n, None, 2, S.LO, S.HI, "mean")
    assert np.array_equal(gf, want[1]) and np.array_equal(_bits(gv), _bits(want[0]))


# ------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors_return_before_any_device_work():
    from nerf_meets_mlx_amd import _native as N
    L = N.lib()
    v, f, n, c = S.mesh("small")
    tv, tn, tf = _dev(v, torch.float32), _dev(n, torch.float32), _dev(f, torch.int32)
    V, F, G = len(v), len(f), 4
    lo, hi = (C.c_float * 3)(*S.LO), (C.c_float * 3)(*S.HI)
    flat = (C.c_float * 3)(1.0, -1.0, -1.0)
    nan = (C.c_float * 3)(float("nan"), 1.0, 1.0)
    ws = poison_(torch.empty(L.nerf_simplify_workspace_bytes(V, F, G), dtype=torch.uint8, device=DEV), NAN_BYTES)
    keys = torch.full((F,), -7, dtype=torch.int64, device=DEV)
    tot = torch.full((3,), -7, dtype=torch.int64, device=DEV)
    ov = sentinel_(torch.empty(V, 3, dtype=torch.float32, device=DEV))
    on = sentinel_(torch.empty(V, 3, dtype=torch.float32, device=DEV))
    of = torch.full((F, 3), SENT32, dtype=torch.int32, device=DEV)
    st = N.stream()
    big = (1 << 24) + 1

    def cluster(verts=tv, normals=tn, V=V, faces=tf, F=F, lo=lo, hi=hi, G=G, ws=ws, keys=keys):
        return L.nerf_simplify_cluster(N.ptr(verts), N.ptr(normals), None, V, N.ptr(faces), F, lo, hi, G, N.ptr(ws), N.ptr(keys), st)

    def count(sk=keys, perm=keys, V=V, faces=tf, F=F, G=G, ws=ws, tot=tot):
        return L.nerf_simplify_count(N.ptr(sk), N.ptr(perm), V, N.ptr(faces), F, G, N.ptr(ws), N.ptr(tot), st)

    def write(V=V, faces=tf, F=F, lo=lo, hi=hi, G=G, placement=1, ws=ws, V2=1, F2=1, ov=ov, on=on, of=of):
        return L.nerf_simplify_write(V, N.ptr(faces), F, lo, hi, G, placement, N.ptr(ws), V2, F2, N.ptr(ov), N.ptr(on), None, None,
                                     N.ptr(of), st)

    for kw in ({"G": 1}, {"G": 513}, {"G": -4}, {"V": -1}, {"F": -1}, {"V": big}, {"F": big}, {"hi": flat}, {"lo": nan}, {"hi": lo},
               {"V": (1 << 21) + 1, "G": 200}):
        assert cluster(**kw) == E_SHAPE, kw
    for kw in ({"verts": None}, {"normals": None}, {"faces": None}, {"ws": None}, {"keys": None}, {"lo": None}, {"hi": None}):
        assert cluster(**kw) == E_NULL, kw
    for kw in ({"G": 1}, {"G": 513}, {"V": -1}, {"F": big}):
        assert count(**kw) == E_SHAPE, kw
    for kw in ({"sk": None}, {"perm": None}, {"faces": None}, {"ws": None}, {"tot": None}):
        assert count(**kw) == E_NULL, kw
    for kw in ({"G": 1}, {"V": big}, {"placement": 2}, {"placement": -1}, {"V2": -1}, {"V2": V + 1}, {"F2": F + 1}, {"F2": -1},
               {"lo": nan}, {"hi": flat}):
        assert write(**kw) == E_SHAPE, kw
    for kw in ({"faces": None}, {"ws": None}, {"ov": None}, {"on": None}, {"of": None}, {"lo": None}):
        assert write(**kw) == E_NULL, kw
    assert b"nerf_simplify_write" in L.nerf_last_error()
    for bad in ((-1, 0, 4), (0, big, 4), (8, 8, 1), (8, 8, 513)):
        assert L.nerf_simplify_workspace_bytes(*bad) == -1
    torch.cuda.synchronize()
    assert bool((keys == -7).all()) and bool((tot == -7).all()) and bool((of == SENT32).all())
    assert unwritten(ov) == ov.numel() and unwritten(on) == on.numel()
    assert bool((ws == NAN_BYTES).all())


# ------------------------------------------------------------------------------------------------ trainers
@pytest.fixture(scope="module")
def march_trainer():
    """hw 48, 2^14-entry tables, march mode, past the grid's warm-up: the trainer of test_gpu_mesh.py's own trainer test."""
    from nerf_meets_mlx_amd.dataset import synthetic
    from nerf_meets_mlx_amd.engine.ngp import NGPTrainer
    imgs, poses, _, _, K = synthetic.make_dataset(48, 48, 8, seed=0, device=DEV)
    tr = NGPTrainer(imgs, poses, K, N_rand=256, n_depth_samples=64, seed=4, device=DEV, log2_hashmap_size=14,
                    occupancy_grid=True, march_steps=1024)
    for _ in range(300):
        tr.train_step()
    vol = tr.density_volume(32)
    thr = float(vol.reshape(-1).quantile(0.9))
    assert float(vol.min()) < thr < float(vol.max())
    return tr, thr


def _rows_of(m):
    rows = torch.zeros(m.verts.shape[0], 11, dtype=torch.float32, device=m.verts.device)
    rows[:, 0:3], rows[:, 3:6], rows[:, 8:11] = m.verts, -m.normals, -m.normals
    return rows


def _same_mesh(a, b):
    return bits_equal(a.verts, b.verts) and torch.equal(a.faces, b.faces) and bits_equal(a.normals, b.normals) \
        and ((a.colors is None and b.colors is None) or bits_equal(a.colors, b.colors))


def test_trainer_extract_mesh_with_simplify_grid(march_trainer, tmp_path):
    from nerf_meets_mlx_amd.engine import mesh as E
    tr, thr = march_trainer
    lo, hi = [-1.5] * 3, [1.5] * 3
    raw = tr.extract_mesh(resolution=32, threshold=thr, colors=False)
    s = tr.extract_mesh(resolution=32, threshold=thr, simplify_grid=8)
    want = E.simplify(raw, 8, lo, hi)
    V, F = s.verts.shape[0], s.faces.shape[0]
    print("V, F", raw.verts.shape[0], raw.faces.shape[0], "->", V, F)
    assert 0 < V < raw.verts.shape[0] and 0 < F < raw.faces.shape[0]
    assert bits_equal(s.verts, want.verts) and torch.equal(s.faces, want.faces) and bits_equal(s.normals, want.normals)
    assert want.colors is None
    assert bits_equal(s.colors, E.vertex_colors(tr._mesh_field()[0], _rows_of(s)))
    assert 0.0 <= float(s.colors.min()) and float(s.colors.max()) <= 1.0
    assert 0 <= int(s.faces.min()) and int(s.faces.max()) == V - 1
    m = tr.extract_mesh(resolution=32, threshold=thr, simplify_grid=8, simplify_placement="mean", colors=False)
    assert m.colors is None and torch.equal(m.faces, s.faces) and not bits_equal(m.verts, s.verts)
    assert _same_mesh(m, E.simplify(raw, 8, lo, hi, "mean"))
    # the reference on the trainer's mesh
    ref = S.simplify(raw.verts.cpu().numpy(), raw.faces.cpu().numpy(), raw.normals.cpu().numpy(), None, 8, lo, hi, "quadric")
    assert np.array_equal(_bits(s.verts.cpu().numpy()), _bits(ref[0])) and np.array_equal(s.faces.cpu().numpy(), ref[1])
    assert np.array_equal(_bits(s.normals.cpu().numpy()), _bits(ref[2]))
    # 0 is the parent's path
    assert _same_mesh(tr.extract_mesh(resolution=32, threshold=thr), tr.extract_mesh(resolution=32, threshold=thr, simplify_grid=0))
    for bad in ({"simplify_grid": 1}, {"simplify_grid": 513}, {"simplify_grid": 8.0}, {"simplify_grid": True},
                {"simplify_grid": 8, "simplify_placement": "median"}):
        with pytest.raises(ValueError):
            tr.extract_mesh(resolution=32, threshold=thr, **bad)
    # PLY round trip
    p = E.write_ply(str(tmp_path / "simplified.ply"), s)
    back = E.read_ply(p)
    assert bits_equal(back.verts, s.verts.cpu()) and torch.equal(back.faces, s.faces.cpu()) and bits_equal(back.normals, s.normals.cpu())
    assert torch.equal(torch.round(back.colors * 255), torch.round(s.colors.cpu().double() * 255).float())


def test_trainer_extract_mesh_tsdf_with_simplify_grid(march_trainer):
    from nerf_meets_mlx_amd.engine import mesh as E
    tr, _ = march_trainer
    lo, hi = [-1.5] * 3, [1.5] * 3
    raw = tr.extract_mesh_tsdf(resolution=32, colors=False)
    assert raw.verts.shape[0] > 0
    s = tr.extract_mesh_tsdf(resolution=32, simplify_grid=8)
    want = E.simplify(raw, 8, lo, hi)
    assert bits_equal(s.verts, want.verts) and torch.equal(s.faces, want.faces) and bits_equal(s.normals, want.normals)
    assert bits_equal(s.colors, E.vertex_colors(tr._mesh_field()[0], _rows_of(s)))
    assert _same_mesh(tr.extract_mesh_tsdf(resolution=32), tr.extract_mesh_tsdf(resolution=32, simplify_grid=0))
    with pytest.raises(ValueError):
        tr.extract_mesh_tsdf(resolution=32, simplify_grid=1)
