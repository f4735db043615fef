"""Mesh ray casting without a GPU: the numpy mirror (tests/_raycast_ref.py) of include/nerf_hip.h "mesh ray casting" held to known
values on the cube, to watertightness on closed meshes, its emulated walk held to the scan over every face bit for bit, its any-hit
walk to face >= 0, its pruning to a cap, its frame to the rasteriser's mirror; the argument checks of engine.mesh and of the C
entries (all of them return before any device work), and the header / binding / Makefile bookkeeping.  The GPU side is held to the
mirror in tests/test_gpu_raycast.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import _distance_ref as D
from tests import _raster_ref as R
from tests import _raycast_ref as RC
from tests import _smooth_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE = -1, -2
ENTRIES = ["nerf_raycast", "nerf_raycast_any"]
F32 = np.float32
CENTRE = [0.0, 0.75, 1.5]                                             # of D.cube(): [-0.5, 0.5]^3 + (0, 0.75, 1.5)
# The mirror's own count on sphere24 (F = 4064) over the 300 rays between D.query_points(.., 300, 5) pairs: 22.05 faces and 68.65
# boxes tested per ray.  The cap is twice that: a walk that stopped pruning would test all 4064.
SPHERE24_MEAN_FACES, SPHERE24_CAP = 22.05, 44.1
# sphere24 at 64 x 64 from the first pose of the rasteriser's tests: the worst |depth| difference between the mirror's ray-cast
# frame and the rasteriser's mirror over the 1274 pixels covered in both is 0.1110 (at one of the 3 pixels where the two pick
# different faces: a silhouette pixel where one sees the front face and the other the back of the sphere behind it).  The bar for
# such pixels is four times it: the rasteriser snaps to 1/256 pixel and works in float32.
FRAME_WORST_DEPTH, FRAME_DEPTH_BAR = 0.1110, 0.444


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


# ------------------------------------------------------------------------------------------------ known values
def test_known_values_on_the_cube():
    v, f = D.cube()
    x = [1.0, 0.0, 0.0]
    rays = np.concatenate([RC.pack([CENTRE], [x]),                                  # from the centre: the right side at 0.5
                           RC.pack([[-2.0, 0.75, 1.5]], [x]),                       # from outside: the near side first
                           RC.pack([[-2.0, 0.75, 1.5]], [x], 2.0),                  # tmin beyond the near side: the far one
                           RC.pack([[-2.0, 0.75, 1.5]], [x], 0.0, 1.0),             # tmax short of it: a miss
                           RC.pack([[-2.0, 0.75, 1.5]], [x], 2.0, 1.0),             # tmin > tmax: a valid ray that misses
                           RC.pack([[-2.0, 0.875, 1.625]], [[2.0, 0.0, 0.0]]),      # d not normalised: t counts in units of d
                           RC.pack([[-2.0, 0.75, 1.5]], [x], 1.5, 1.5)])            # the window closed on the hit itself
    for t, face, bary in (RC.brute_force(rays, v, f), RC.Caster(v, f).cast(rays)[:3]):
        assert t.tolist()[:3] == [0.5, 1.5, 2.5] and np.isposinf(t[3:5]).all() and t[5] == 0.75 and t[6] == 1.5
        # x = +0.5 is the faces 10 = (1, 3, 5) and 11 = (3, 7, 5), x = -0.5 the faces 8 = (0, 4, 2) and 9 = (2, 4, 6); the centre
        # ray meets their shared diagonal, where the lower index wins
        assert face.tolist() == [10, 8, 10, -1, -1, 9, 8]
        assert bary[[0, 1, 2, 6]].tolist() == [[0.5, 0.5]] * 4 and np.isnan(bary[3:5]).all()
        # the hit point is a + wb (b - a) + wc (c - a)
        g = f[face[5]]
        p = v[g[0]] + bary[5, 0] * (v[g[1]] - v[g[0]]) + bary[5, 1] * (v[g[2]] - v[g[0]])
        assert p.tolist() == [-0.5, 0.875, 1.625]
    bad = RC.bad_rays()
    assert len(bad) == 7 and not RC.valid_rays(bad).any() and RC.valid_rays(rays).all()
    for t, face, bary in (RC.brute_force(bad, v, f), RC.Caster(v, f).cast(bad)[:3]):
        assert (_bits(t) == 0x7FC00000).all() and (face == -1).all() and (_bits(bary) == 0x7FC00000).all()
    assert not RC.Caster(v, f).cast(bad)[3].any() and not RC.Caster(v, f).any(bad).any()


# ------------------------------------------------------------------------------------------------ watertightness
@pytest.mark.parametrize("name", ["sphere12", "sphere24", "cube"])
def test_no_ray_from_inside_a_closed_mesh_misses(name):
    v, f = RC.MESHES[name]()
    v, f = np.asarray(v, F32), np.asarray(f, np.int32)
    ctr = np.array(CENTRE if name == "cube" else S.CENTRE, np.float64)
    ok, a, b, c, _ = D.corners(v, f)
    assert ok.all()
    mids = np.concatenate([(a + b) * F32(0.5), (b + c) * F32(0.5), (c + a) * F32(0.5)])
    rng = np.random.default_rng(17)
    f2 = np.concatenate([f, f])
    for off in ([0.0, 0.0, 0.0], [0.125, -0.0625, 0.09375], [-0.21, 0.13, -0.17]):
        o = (ctr + off).astype(F32)
        targets = np.concatenate([v, mids, (o + rng.standard_normal((300, 3))).astype(F32)])
        rays = RC.pack(np.tile(o, (len(targets), 1)), targets - o)
        t, face, bary = RC.brute_force(rays, v, f)
        assert (face >= 0).all() and np.isfinite(t).all() and (t > 0).all(), (name, off, int((face < 0).sum()))
        # a ray at a vertex or an edge midpoint arrives there at t = 1 up to the rounding of the midpoint and of d: all of them on
        # the cube, which is convex; the spheres are marching-cubes surfaces with dents, where some rays meet a face in front of
        # their target or graze past it to one behind
        arrived = np.abs(t[:len(v) + len(mids)] - 1.0) < 1e-5
        assert arrived.all() if name == "cube" else arrived.mean() > 0.5
        t2, face2, bary2 = RC.brute_force(rays, v, f2)                 # every face twice: the lower index wins every hit
        assert np.array_equal(_bits(t2), _bits(t)) and np.array_equal(face2, face) and np.array_equal(_bits(bary2), _bits(bary))


# ------------------------------------------------------------------------------------------------ the walk
@pytest.mark.parametrize("name", sorted(RC.MESHES))
def test_the_walk_equals_the_brute_force_bit_for_bit(name):
    v, f, rays, brute, walk, hit = RC.case(name)
    good = RC.valid_rays(rays)
    assert len(rays) == 300 + 14 + 96 + (24 if D.corners(v, f)[0].any() else 0) + 7 + 1 and (~good).sum() == 7
    for got, want in zip(walk[:3], brute):
        bad = (_bits(got) != _bits(want)) if got.dtype == F32 else (got != want)
        assert not bad.any(), (name, np.nonzero(bad)[0][:6])
    t, face, bary, visits = walk
    assert np.array_equal(hit != 0, face >= 0)                         # any-hit
    assert (_bits(t[~good]) == 0x7FC00000).all() and (face[~good] == -1).all() and not visits[~good].any()
    miss = good & (face < 0)
    assert np.isposinf(t[miss]).all() and (_bits(bary[miss]) == 0x7FC00000).all()
    got = face >= 0
    assert np.isfinite(t[got]).all() and np.isfinite(bary[got]).all() and D.corners(v, f)[0][face[got]].all()
    assert (t[got] >= rays[got, 6]).all() and (t[got] <= rays[got, 7]).all() and (_bits(t[got]) >= 0).all()
    assert (visits[good, 1] >= 1).all() and (visits[good, 0] <= max(len(f), 1)).all()
    if not D.corners(v, f)[0].any():
        assert not got.any() and (visits[good] == (0, 1)).all()        # the empty root is the one box tested
    if name == "doubled":
        assert got.any() and (face[got] < len(f) // 2).all()
    if name == "cube":                                                 # the rays in the planes of its sides are among them
        plane = rays[314:410]
        assert ((plane[:, 3:6] == 0).sum(1) == 2).all() and got[314:410].sum() > 0


def test_a_cast_tests_a_small_share_of_the_faces():
    """Agreement with the brute force cannot see a walk that stopped pruning: it would only be slower."""
    v, f, rays, _, (t, face, bary, visits), _ = RC.case("sphere24")
    mean = visits[:300].mean(0)
    print("sphere24: mean faces tested", mean[0], "of", len(f), "boxes tested", mean[1])
    assert len(f) == 4064 and mean[0] <= SPHERE24_CAP < 0.011 * len(f)
    assert abs(mean[0] - SPHERE24_MEAN_FACES) < 0.01                   # the figure DESIGN.md section 42 quotes
    # any-hit tests no more than the nearest hit does
    c = RC.Caster(v, f)
    assert all(c.one(r, any_hit=True)[1] <= n for r, n in zip(rays[:40], visits[:40, 0]))


# ------------------------------------------------------------------------------------------------ against the rasteriser
def test_the_frame_agrees_with_the_rasterisers_mirror_up_to_silhouettes():
    H = W = 64
    v, f, c2w, K, (face, bary, depth, acc, visits) = RC.sphere24_frame()
    _, _, rf, rb, rd, ra = R.render(v, f, R.view_of(c2w, K), H, W, 0.01)
    rf, rd, ra = rf.reshape(H, W), rd.reshape(H, W), ra.reshape(H, W)
    assert face.shape == (H, W) and bary.shape == (H, W, 2) and depth.dtype == F32 and set(np.unique(acc)) == {0.0, 1.0}
    assert ((face >= 0) == (acc == 1)).all() and (depth[acc == 0] == 0).all() and (bary[acc == 0] == 0).all()
    cov_r, cov_c = ra > 0, acc > 0
    assert 1000 < cov_c.sum() < 2000
    # where the two disagree on coverage, the raster frame has an uncovered 8-neighbour: a silhouette pixel
    pad = np.pad(~cov_r, 1, constant_values=True)
    edge = np.zeros((H, W), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                edge |= pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    differ = cov_r != cov_c
    assert edge[differ].all(), int(differ.sum())
    both = cov_r & cov_c
    dd = np.abs(rd.astype(np.float64) - depth.astype(np.float64))
    other = both & (rf != face)
    same = both & (rf == face)
    print("sphere24 64 x 64: coverage differs at", int(differ.sum()), "pixels, the face at", int(other.sum()), "of", int(both.sum()),
          "; worst depth difference", dd[both].max(), "(same face:", dd[same].max(), ")")
    assert (dd[other] <= FRAME_DEPTH_BAR).all()
    assert abs(dd[both].max() - FRAME_WORST_DEPTH) < 1e-4              # the figure DESIGN.md section 42 quotes
    assert other.sum() <= 0.01 * both.sum()


# ------------------------------------------------------------------------------------------------ host-side API
def test_arguments_are_checked():
    from nerf_meets_mlx_amd.engine import mesh as E
    v, f = (torch.from_numpy(a.copy()) for a in S.sphere(12))
    good = E.Mesh(v, f, torch.zeros_like(v), None)
    rays = torch.zeros(5, 11)
    inf = float("inf")
    assert E.check_raycast_args(good, S.LO, S.HI) == (S.LO, S.HI, inf)
    assert E.check_raycast_args(good, S.LO, S.HI, rays, 6) == (S.LO, S.HI, 6.0)
    for lo, hi in (([0.0] * 3, [0.0] * 3), ([0.0] * 3, [1.0, 1.0, float("nan")]), ([0.0] * 2, [1.0] * 2), (S.HI, S.LO)):
        with pytest.raises(ValueError, match="box"):
            E.check_raycast_args(good, lo, hi)
        with pytest.raises(ValueError, match="box"):
            E.MeshRaycast(good, lo, hi)
    for m in (good._replace(verts=v.double()), good._replace(faces=f.long()), (v, f), None):
        with pytest.raises(ValueError):
            E.check_raycast_args(m, S.LO, S.HI)
        with pytest.raises(ValueError):
            E.MeshRaycast(m, S.LO, S.HI)
        with pytest.raises(ValueError):
            E.raycast_frame(m, np.eye(4)[:3], np.eye(3), 4, 4)
    for r in (rays.double(), rays[:, :8], rays.numpy(), rays.t().contiguous().t(), torch.zeros(11), torch.zeros(5, 3)):
        with pytest.raises(ValueError, match="rays"):
            E.check_raycast_args(good, S.LO, S.HI, r)
    for far in (float("nan"), 0.0, -1.0, None, "6", True, -inf):
        with pytest.raises(ValueError, match="far"):
            E.check_raycast_args(good, S.LO, S.HI, far=far)
    with pytest.raises(ValueError, match="far"):
        E.render_mesh_rays(good._replace(colors=torch.zeros_like(v)), np.eye(4)[:3], np.eye(3), 4, 4, far=float("nan"))
    with pytest.raises(ValueError, match="bvh"):
        E.MeshRaycast(good, S.LO, S.HI, bvh=object())
    for H, W in ((0, 4), (4, 16385), (2.5, 4)):
        with pytest.raises(ValueError, match="raster"):
            E.raycast_frame(good, np.eye(4)[:3], np.eye(3), H, W)
    with pytest.raises(ValueError, match="near"):
        E.raycast_frame(good, np.eye(4)[:3], np.eye(3), 4, 4, near=0.0)
    with pytest.raises(ValueError, match="chunk"):
        E.raycast_frame(good, np.eye(4)[:3], np.eye(3), 4, 4, chunk=0)
    with pytest.raises(ValueError, match="caster"):
        E.raycast_frame(good, np.eye(4)[:3], np.eye(3), 4, 4, caster=object())
    with pytest.raises(ValueError, match="needs a texture"):
        E.render_mesh_rays(good, np.eye(4)[:3], np.eye(3), 4, 4)
    # pack_rays is torch plumbing and runs anywhere
    o, d = torch.tensor([[0.0, 1.0, 2.0], [3.0, 4.0, 5.0]]), torch.tensor([[1.0, 0.0, 0.0], [0.0, 2.0, 0.0]])
    p = E.pack_rays(o, d)
    assert p.shape == (2, 11) and p.dtype == torch.float32 and E.RAY_STRIDE == 11
    assert torch.equal(p[:, :3], o) and torch.equal(p[:, 3:6], d) and p[:, 6].tolist() == [0.0, 0.0] and p[:, 7].tolist() == [inf, inf]
    assert not p[:, 8:].any()
    p = E.pack_rays(o, d, 0.5, torch.tensor([2.0, 3.0]))
    assert p[:, 6].tolist() == [0.5, 0.5] and p[:, 7].tolist() == [2.0, 3.0]
    assert np.array_equal(p.numpy()[:, :8], RC.pack(o.numpy(), d.numpy(), 0.5, np.array([2.0, 3.0]))[:, :8])
    for bad_o, bad_d in ((o.double(), d), (o, d[:1]), (o[:, :2], d), (o.numpy(), d)):
        with pytest.raises(ValueError):
            E.pack_rays(bad_o, bad_d)
    assert E.RAYCAST_SLACK == RC.SLACK == 2.0 ** -30 and isinstance(E.RAYCAST_SORTED_QUERY, bool)
    assert E.RayHits._fields == ("t", "face", "bary", "visits")


def test_trainer_methods_and_mesh_tool_options():
    from nerf_meets_mlx_amd.engine.ngp import NGPTrainer
    from nerf_meets_mlx_amd.engine.trainer import Trainer
    E = inspect.Parameter.empty

    def sig(cls, name):
        return [(p.name, p.default) for p in inspect.signature(getattr(cls, name)).parameters.values()][1:]

    # the existing parameter lists are unchanged
    assert sig(Trainer, "render_mesh") == [("mesh", E), ("c2w", E), ("texture", None), ("background", None)]
    assert sig(Trainer, "mesh_psnr") == [("mesh", E), ("c2w", E), ("gt", E), ("texture", None), ("background", None)]
    assert sig(Trainer, "remesh") == [("mesh", E), ("resolution", 256), ("aabb", None), ("beta", 2.0), ("min_component", 0),
                                      ("largest_only", False), ("opening_radius", 0)]
    assert sig(Trainer, "signed_distance") == [("mesh", E), ("points", E), ("aabb", None), ("beta", 2.0)]
    assert [n for n, _ in sig(Trainer, "mesh_distance")] == ["mesh", "other", "n", "tau", "seed", "aabb"]
    assert sig(NGPTrainer, "render_depth") == [("c2w", E)]
    # the new methods
    assert sig(Trainer, "raycast_mesh")[:2] == [("mesh", E), ("c2w", E)] and all(d is not E for _, d in sig(Trainer, "raycast_mesh")[2:])
    assert sig(NGPTrainer, "mesh_depth_error")[:3] == [("mesh", E), ("c2w", E), ("acc_min", 0.5)]
    assert all(d is not E for _, d in sig(NGPTrainer, "mesh_depth_error")[3:]) and "raycast_mesh" not in vars(NGPTrainer)
    import importlib.util
    spec = importlib.util.spec_from_file_location("ngp_mesh_tool_raycast", os.path.join(ROOT, "tools", "ngp_mesh.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert tool.parser().parse_args([]).raycast is False and tool.parser().parse_args(["--raycast"]).raycast is True


def test_c_entries_refuse_before_any_device_work():
    from nerf_meets_mlx_amd import _native as N
    L = N.lib()
    p = C.c_void_p(4096)                                               # never dereferenced: every call below is refused
    odd = C.c_void_p(4096 + 8)
    big = (1 << 24) + 1
    lo, hi = (C.c_float * 3)(*S.LO), (C.c_float * 3)(*S.HI)
    nan_hi = (C.c_float * 3)(1.0, float("nan"), 1.0)

    def cast(rays=p, n=5, verts=p, V=4, faces=p, F=4, lo=lo, hi=hi, ws=p, t=p, face=p, bary=p, visits=p):
        return L.nerf_raycast(rays, n, verts, V, faces, F, lo, hi, ws, t, face, bary, visits, None)

    def any_hit(rays=p, n=5, verts=p, V=4, faces=p, F=4, lo=lo, hi=hi, ws=p, hit=p):
        return L.nerf_raycast_any(rays, n, verts, V, faces, F, lo, hi, ws, hit, None)

    shapes = [{"V": big}, {"V": -1}, {"F": big}, {"F": -1}, {"n": -1}, {"n": (1 << 30) + 1}, {"ws": odd}, {"lo": hi, "hi": lo},
              {"hi": nan_hi}, {"lo": lo, "hi": lo}]
    for fn, name in ((cast, b"nerf_raycast"), (any_hit, b"nerf_raycast_any")):
        for kw in shapes:
            assert fn(**kw) == E_SHAPE, (name, kw)
            assert name in L.nerf_last_error()
        # a bad box or size is refused even where nothing would be launched; nothing to do is no error, whatever the pointers
        assert fn(n=0, F=big) == E_SHAPE and fn(n=0, hi=nan_hi) == E_SHAPE and fn(n=0, ws=odd) == E_SHAPE
        assert fn(lo=None) == E_NULL and fn(hi=None) == E_NULL
    for kw in ({"rays": None}, {"verts": None}, {"faces": None}, {"ws": None}, {"t": None}, {"face": None}, {"bary": None},
               {"visits": None}, {"ws": None, "F": 0}):
        assert cast(**kw) == E_NULL, kw
    for kw in ({"rays": None}, {"verts": None}, {"faces": None}, {"ws": None}, {"hit": None}, {"ws": None, "F": 0}):
        assert any_hit(**kw) == E_NULL, kw
    assert cast(n=0, rays=None, ws=None, t=None, face=None, bary=None, visits=None) == 0
    assert any_hit(n=0, rays=None, ws=None, hit=None) == 0


def test_header_section_bindings_and_makefile():
    from nerf_meets_mlx_amd import _native
    from nerf_meets_mlx_amd.engine import mesh as E
    text = open(os.path.join(ROOT, "include", "nerf_hip.h")).read()
    start = text.index("/* ---------------------------------------------------------------- mesh ray casting (no reference counterpart)")
    wind = text.index("mesh winding number (no reference counterpart)")
    nxt = text.index("/* ----", start + 3)
    assert text.index("/* ----", wind) == start                        # directly behind "mesh winding number"
    assert nxt == text.index("/* ---------------------------------------------------------------- texture atlas (no reference counterpart)")
    section = text[start + 3:nxt]
    decl = re.sub(r"/\*.*?\*/", "", "/*" + section, flags=re.S)
    assert sorted(set(re.findall(r"\b(nerf_[a-z_]+)\s*\(", decl))) == ENTRIES
    lib = _native.lib()
    for e in ENTRIES:
        assert e in _native.SIGNATURES and hasattr(lib, e)
    assert len(_native.SIGNATURES["nerf_raycast"][1]) == 14 and len(_native.SIGNATURES["nerf_raycast_any"][1]) == 11
    assert lib.nerf_abi_version() == 3 and "#define NERF_ABI_VERSION 3" in text
    flat = re.sub(r"\s+", " ", section.replace("\n * ", " ").replace("\n *", " "))
    for word in ("Woop, Benthin and Wald 2013", "the lowest axis on a tie", "swapped if d[kz] < 0", "Sx = d[kx] / d[kz]",
                 "U = Cx By - Cy Bx, V = Ax Cy - Ay Cx, W = Bx Ay - By Ax", "zeros are inclusive", "det = (U + V) + W", "det == 0 misses",
                 "t64 = ((U Az + V Bz) + W Cz) / det", "t = (float)t64 + 0.0f", "tmin <= t and t <= tmax", "(float)(V / det)",
                 "exact negatives", "no ray slips between them", "(bits of t) 2^32 + f", "the lowest face index on equal t",
                 "(+inf, -1, NaN, NaN)", "NaN (0x7FC00000)", "tmin > tmax is a valid ray that misses", "columns 8-10 are not read",
                 "the left one on a tie", "it is tested again", "eta = 2^-30 S", "no 0 inf is ever formed", "strictly greater than the best t",
                 "a lower face index may still tie", "proof", "rounding is monotone", "convex combination", "no atomics, no LDS, no scratch",
                 "one build serves any number of chunks", "NERF_ABI_VERSION stays 3", "Not done", "no all-hits or parity counting",
                 "exact at the near plane", "no packet or wave-cooperative traversal", "no better splits than the Morton median"):
        assert word in flat, word
    for other, word in (("mesh BVH (no reference counterpart)", "no ray casting"),
                        ("mesh winding number (no reference counterpart)", "still no ray casting")):
        at = text.index(other)
        assert word in re.sub(r"\s+", " ", text[at:text.index("/* ----", at)].replace("\n * ", " "))
    csrc = os.path.join(ROOT, "nerf_meets_mlx_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    srcs = next(ln for ln in mk.splitlines() if ln.startswith("SRCS"))
    assert "raycast.hip" in srcs.split() and "bvh.hip" in srcs.split() and "winding.hip" in srcs.split()
    assert not re.search(r"FLAGS_raycast", mk) and "-ffp-contract=off" in mk     # the default flags
    src = open(os.path.join(csrc, "raycast.hip")).read()
    assert sorted(set(re.findall(r"\b(\w+_kernel)\b", src))) == ["raycast_kernel"]
    assert not re.search(r"\batomic\w*\(", src) and "__shared__" not in src      # no atomics at all, no LDS
    assert '#include "bvh_tree.h"' in src and '#include "distance.h"' in src
    for shared in ("tree_leaf_faces(", "dist_load(", "points_check(", "ws_aligned16_check(", "box_abs(", "NERF_TRY(", "mesh_check(",
                   "box_check(", "DIST_LAUNCH("):
        assert shared in src, shared
    # bvh.hip's four kernels and winding.hip's two are as they were
    assert sorted(set(re.findall(r"\b(\w+_kernel)\(", open(os.path.join(csrc, "bvh.hip")).read()))) == \
        ["bvh_closest_kernel", "bvh_keys_kernel", "bvh_leaves_kernel", "bvh_query_kernel"]
    assert sorted(set(re.findall(r"\b(\w+_kernel)\(", open(os.path.join(csrc, "winding.hip")).read()))) == \
        ["wind_leaves_kernel", "wind_query_kernel"]
    module = open(os.path.join(ROOT, "nerf_meets_mlx_amd", "engine", "mesh", "raycast.py")).read()
    for name in ("MeshRaycast", "RayHits", "pack_rays", "raycast_frame", "render_mesh_rays", "check_raycast_args"):
        assert hasattr(E, name) and name in module
    assert "_render(" in module and "lib().nerf_raster_shade" not in module          # the shading path is reused, not copied
    assert "MeshRaycast" in E.__doc__ and "distance (sample_surface, MeshIndex, mesh_distance)" in E.__doc__
    log = open(os.path.join(ROOT, "profiles", "raycast_resources.log")).read()
    assert "raycast_kernel" in log and "scratch" in log.lower()
