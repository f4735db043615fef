"""The mesh rasteriser without a GPU: the header / binding / Makefile / engine / tool bookkeeping, the argument checks of the C ABI
(they return before any device work, so they run here) and of engine.mesh, and the properties of the rule of include/nerf_hip.h
"mesh rendering" on its numpy statement tests/_raster_ref.py: watertight coverage, independence of face order, perspective-correct
interpolation, hidden surfaces, dropped faces and back-face culling.  The kernels are held to that reference bit for bit in
tests/test_gpu_raster.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import _raster_ref as R
from tests import _smooth_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE = -1, -2
ENTRIES = ["nerf_raster_clear", "nerf_raster_draw", "nerf_raster_resolve", "nerf_raster_shade"]
KERNELS = ["raster_clear_kernel", "raster_draw_kernel", "raster_resolve_kernel", "raster_shade_kernel"]
NEAR = 0.01
POSES = [R.look_at(S.CENTRE + [2.6, 1.1, 2.2], S.CENTRE), R.look_at(S.CENTRE + [-2.0, -0.7, 2.4], S.CENTRE + [0.3, 0.1, 0.0])]
MESHES = {"tetrahedron": S.tetrahedron, "sphere12": lambda: S.sphere(12), "sphere24": lambda: S.sphere(24)}


def _lib():
    from nerf_meets_mlx_amd import _native
    return _native.lib()


# ------------------------------------------------------------------------------------------------ bookkeeping
def test_header_section_bindings_and_makefile():
    from nerf_meets_mlx_amd import _native
    from nerf_meets_mlx_amd.engine import mesh as E
    text = open(os.path.join(ROOT, "include", "nerf_hip.h")).read()
    start = text.index("/* ---------------------------------------------------------------- mesh rendering (no reference counterpart)")
    banners = [m.start() for m in re.finditer(r"/\* ----", text)]
    k = banners.index(start)
    assert text[banners[k - 1]:].startswith("/* ---------------------------------------------------------------- texture atlas")
    assert text[banners[k + 1]:].startswith("/* ---------------------------------------------------------------- fused renderer (a14 / a18)")
    section = text[start:banners[k + 1]]
    decl = re.sub(r"/\*.*?\*/", "", section, flags=re.S)
    assert sorted(set(re.findall(r"\b(nerf_raster_[a-z_]+)\s*\(", decl))) == ENTRIES and len(ENTRIES) <= 5
    assert sorted(set(re.findall(r"\b(nerf_raster_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))) == ENTRIES
    assert f"#define NERF_RASTER_SMALL_MAX {E.RASTER_SMALL_MAX}" in decl and R.SMALL_MAX == E.RASTER_SMALL_MAX
    assert "#define NERF_ABI_VERSION 3" in text
    lib = _lib()
    for e in ENTRIES:
        assert e in _native.SIGNATURES and hasattr(lib, e)
    assert sorted(s for s in _native.SIGNATURES if s.startswith("nerf_raster_")) == ENTRIES
    for word in ("rintf(u * 256.0f)", "Ea + Eb + Ec = S exactly", "Q = (qa + qb) + qc", "z = (float)S / Q", "atomicMin", "2^20", "2^28",
                 "Not done", "clipping", "antialiasing", "mipmapped", "tile binning", "transparency"):
        assert word in section, word
    mk = open(os.path.join(ROOT, "nerf_meets_mlx_amd", "csrc", "Makefile")).read()
    assert "raster.hip" in next(ln for ln in mk.splitlines() if ln.startswith("SRCS")).split()
    assert "raster.h" in next(ln for ln in mk.splitlines() if ln.startswith("HDRS")).split()
    src = open(os.path.join(ROOT, "nerf_meets_mlx_amd", "csrc", "raster.hip")).read()
    assert sorted(set(re.findall(r"\b(\w+_kernel)\(", src))) == KERNELS
    code = re.sub(r"//.*", "", src + open(os.path.join(ROOT, "nerf_meets_mlx_amd", "csrc", "raster.h")).read())
    assert "atomicMin" in code and not re.search(r"atomic\w*\([^)]*float", code)          # no float atomics
    assert set(re.findall(r"\batomic\w+", code)) == {"atomicMin", "atomicAdd"}


def test_engine_and_trainer_signatures():
    from nerf_meets_mlx_amd.engine import mesh as E
    from nerf_meets_mlx_amd.engine.ngp import NGPTrainer
    from nerf_meets_mlx_amd.engine.trainer import Trainer
    assert E.MeshFrame._fields == ("rgb", "depth", "acc", "face", "bary")
    p = inspect.signature(E.rasterize).parameters
    assert list(p)[:8] == ["mesh", "c2w", "K", "H", "W", "near", "cull_backfaces", "mark"]
    assert (p["cull_backfaces"].default, p["mark"].default, p["small_max"].default) == (False, None, E.RASTER_SMALL_MAX)
    p = inspect.signature(E.render_mesh).parameters
    assert list(p)[:10] == ["mesh", "c2w", "K", "H", "W", "texture", "background", "near", "cull_backfaces", "mark"]
    assert (p["texture"].default, p["background"].default, p["cull_backfaces"].default, p["mark"].default) == (None, None, False, None)
    assert list(inspect.signature(Trainer.render_mesh).parameters) == ["self", "mesh", "c2w", "texture", "background"]
    assert list(inspect.signature(Trainer.mesh_psnr).parameters) == ["self", "mesh", "c2w", "gt", "texture", "background"]
    assert NGPTrainer.render_mesh is Trainer.render_mesh and NGPTrainer.mesh_psnr is Trainer.mesh_psnr
    assert E.check_raster_args(48, np.int64(64), 2, True, 0) == (48, 64, 2.0, True, 0)


def test_mesh_tool_knows_the_raster_kernels_and_flags(tmp_path, capsys):
    import argparse
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("ngp_mesh_tool", os.path.join(ROOT, "tools", "ngp_mesh.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    path = tmp_path / "trace.csv"
    with open(path, "w") as fh:
        fh.write('"Kernel_Name","Start_Timestamp","End_Timestamp","Grid_Size_X"\n')
        for i, k in enumerate(KERNELS):
            for rep in range(2):
                fh.write(f'"nerf::(anonymous namespace)::{k}(float const*, int)",{1000 * i},{1000 * i + 500 + 1000 * rep},{256 * (i + 1)}\n')
    tool.stats(argparse.Namespace(stats=str(path), from_=None, out=None))
    recs = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert sorted(r["kernel"] for r in recs) == KERNELS and all(r["launches"] == 2 and r["avg_us"] == 1.0 for r in recs)
    assert tool._raster_bytes("raster_clear_kernel", 1000) == 8000 and tool._raster_bytes("raster_resolve_kernel", 10) == 280
    # with the measuring run's lines the draws come apart by mesh and small_max, in launch order
    lines = tmp_path / "run.jsonl"
    lines.write_text(json.dumps({"tool": "ngp_mesh render", "F": 500, "draw_launch_small_max": [16, 0]}) + "\n")
    tool.stats(argparse.Namespace(stats=str(path), from_=str(lines), out=None))
    recs = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert {"raster_draw_kernel F=500 small_max=16", "raster_draw_kernel F=500 small_max=0"} <= {r["kernel"] for r in recs}
    a = tool.parser().parse_args(["--render", "--small-max", "0", "--small-max", "64", "--render-dir", "x"])
    assert a.render and a.small_max == [0, 64] and a.render_dir == "x"
    a = tool.parser().parse_args([])
    assert not a.render and a.small_max is None and a.render_dir is None


# ------------------------------------------------------------------------------------------------ argument errors
def test_every_argument_error_returns_before_device_work():
    """Without a device the first launch would fail with NERF_E_HIP: every refusal below is NERF_E_SHAPE or NERF_E_NULL, so it was
    made before any device work.  The device pointers are never dereferenced."""
    lib = _lib()
    p = C.c_void_p(4096)
    big = (1 << 24) + 1
    good = R.view_of(POSES[0], R.intrinsics(48, 64))

    def view(x=good):
        return None if x is None else np.ascontiguousarray(x, np.float32).ctypes.data_as(C.POINTER(C.c_float))

    def bad_view(k, value):
        v = good.copy()
        v[k] = value
        return v

    def clear(keys=p, H=48, W=64, stats=p):
        return lib.nerf_raster_clear(keys, H, W, stats, None)

    def draw(verts=p, V=10, faces=p, F=9, base=0, vw=good, H=48, W=64, near=0.5, cull=0, sm=16, keys=p, stats=p):
        return lib.nerf_raster_draw(verts, V, faces, F, base, view(vw), H, W, near, cull, sm, keys, stats, None)

    def resolve(keys=p, verts=p, V=10, faces=p, F=9, vw=good, H=48, W=64, near=0.5, face=p, bary=p, depth=p, acc=p):
        return lib.nerf_raster_resolve(keys, verts, V, faces, F, view(vw), H, W, near, face, bary, depth, acc, None)

    def shade(face=p, bary=p, faces=p, V=10, F=9, colors=p, rgb_in=None, bg=p, per_pixel=0, H=48, W=64, rgb=p):
        return lib.nerf_raster_shade(face, bary, faces, V, F, colors, rgb_in, bg, per_pixel, H, W, rgb, None)

    sizes = [{"H": 0}, {"W": 0}, {"H": 16385}, {"W": 16385}, {"H": -1}]
    mesh = [{"V": -1}, {"V": big}, {"F": -1}, {"F": big}]
    cam = [{"near": 0.0}, {"near": -1.0}, {"near": float("inf")}, {"near": float("nan")}, {"vw": bad_view(3, np.nan)},
           {"vw": bad_view(12, np.inf)}, {"vw": bad_view(0, -np.inf)}]
    shape = {"nerf_raster_clear": [lambda kw=kw: clear(**kw) for kw in sizes],
             "nerf_raster_draw": [lambda kw=kw: draw(**kw) for kw in sizes + mesh + cam + [
                 {"base": -1}, {"base": (1 << 24) - 8}, {"F": 1 << 24, "base": 1}, {"cull": 2}, {"cull": -1}, {"sm": -1}, {"sm": (1 << 30) + 1}]],
             "nerf_raster_resolve": [lambda kw=kw: resolve(**kw) for kw in sizes + mesh + cam],
             "nerf_raster_shade": [lambda kw=kw: shade(**kw) for kw in sizes + mesh + [{"per_pixel": 2}, {"per_pixel": -1}]]}
    for name, calls in shape.items():
        for k, call in enumerate(calls):
            assert call() == E_SHAPE, (name, k)
            assert name.encode() in lib.nerf_last_error(), (name, k, lib.nerf_last_error())
    null = {"nerf_raster_clear": [lambda: clear(keys=None), lambda: clear(stats=None)],
            "nerf_raster_draw": [lambda kw=kw: draw(**kw) for kw in ({"verts": None}, {"faces": None}, {"vw": None}, {"keys": None},
                                                                   {"stats": None}, {"F": 0, "keys": None})],
            "nerf_raster_resolve": [lambda kw=kw: resolve(**kw) for kw in ({"keys": None}, {"verts": None}, {"faces": None}, {"vw": None},
                                                                         {"face": None}, {"bary": None}, {"depth": None}, {"acc": None})],
            "nerf_raster_shade": [lambda kw=kw: shade(**kw) for kw in ({"face": None}, {"bary": None}, {"faces": None}, {"bg": None},
                                                                     {"rgb": None}, {"colors": None}, {"rgb_in": p})]}
    for name, calls in null.items():
        for k, call in enumerate(calls):
            assert call() == E_NULL, (name, k)
            assert name.encode() in lib.nerf_last_error(), (name, k)
    # nothing to draw is no error and needs neither a mesh nor a device; the limits themselves are accepted
    assert draw(F=0, faces=None, verts=None, V=0) == 0 and draw(F=0, H=16384, W=16384, sm=1 << 30, base=1 << 24) == 0
    assert draw(F=0, sm=0, cull=1, near=1e-30) == 0


def test_engine_argument_checks():
    from nerf_meets_mlx_amd.engine import mesh as E
    v, f = (torch.from_numpy(a.copy()) for a in S.sphere(12))
    n = torch.zeros_like(v)
    good = E.Mesh(v, f, n, torch.zeros_like(v))
    K = R.intrinsics(48, 64)
    for kw, word in (({"H": 0}, "H"), ({"H": 16385}, "H"), ({"W": True}, "W"), ({"W": 4.0}, "W"), ({"near": 0.0}, "near"),
                     ({"near": float("nan")}, "near"), ({"near": 1e-60}, "near"), ({"near": "1"}, "near"), ({"near": True}, "near"),
                     ({"cull_backfaces": 1}, "cull_backfaces"), ({"small_max": -1}, "small_max"), ({"small_max": (1 << 30) + 1}, "small_max"),
                     ({"small_max": 2.0}, "small_max")):
        with pytest.raises(ValueError, match=word):
            E.check_raster_args(**kw)
        args = {"H": 48, "W": 64, **kw}
        with pytest.raises(ValueError, match=word):
            E.rasterize(good, POSES[0], K, **args)
        with pytest.raises(ValueError, match=word):
            E.render_mesh(good, POSES[0], K, **args)
    bad = [good._replace(verts=v.double()), good._replace(faces=f.long()), good._replace(colors=n[:, :2]), good._replace(faces=f[:, :2]), (v, f)]
    for m in bad:
        with pytest.raises(ValueError):
            E.rasterize(m, POSES[0], K, 48, 64)
        with pytest.raises(ValueError):
            E.render_mesh(m, POSES[0], K, 48, 64)
    with pytest.raises(ValueError, match="needs a texture"):
        E.render_mesh(good._replace(colors=None), POSES[0], K, 48, 64)
    for c2w, Kx in ((np.zeros((2, 4)), K), (np.stack([POSES[0], POSES[0]]), K), (POSES[0], np.eye(4)), (POSES[0] * np.nan, K)):
        with pytest.raises(ValueError):
            E.rasterize(good, c2w, Kx, 48, 64)
    for bg in (torch.zeros(4), torch.zeros(48 * 64, 4), torch.zeros(47 * 64, 3)):
        with pytest.raises(ValueError, match="background"):
            E.render_mesh(good, POSES[0], K, 48, 64, background=bg)
    with pytest.raises(ValueError):                                       # there is no CPU path
        E.render_mesh(good, POSES[0], K, 48, 64)


def test_no_faces_gives_the_background_without_a_launch():
    from nerf_meets_mlx_amd.engine import mesh as E
    v = torch.from_numpy(S.tetrahedron()[0].copy())
    m = E.Mesh(v, torch.zeros(0, 3, dtype=torch.int32), torch.zeros_like(v), torch.zeros_like(v))
    K = R.intrinsics(5, 7)
    stages = []
    fr = E.render_mesh(m, POSES[0], K, 5, 7, mark=stages.append)             # (CPU tensors: any launch would raise)
    assert stages == [] and fr.rgb.shape == (5, 7, 3) and bool((fr.rgb == 1.0).all())         # white, the renderer's default
    assert bool((fr.face == -1).all()) and fr.face.dtype == torch.int32 and not fr.depth.any() and not fr.acc.any() and not fr.bary.any()
    bg = torch.rand(35, 3)
    assert torch.equal(E.render_mesh(m, POSES[0], K, 5, 7, background=bg).rgb, bg.reshape(5, 7, 3))
    assert torch.equal(E.render_mesh(m, POSES[0], K, 5, 7, background=[0.5, 0.25, 0.0]).rgb[4, 6], torch.tensor([0.5, 0.25, 0.0]))
    assert E.rasterize(m, POSES[0], K, 5, 7)[4].tolist() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ properties of the rule
def _rays(c2w, K, H, W):
    """(origin [3], directions [H, W, 3] with camera z = -1): the rays of the pixel centres; a point at depth zc is o + zc d."""
    py, px = np.mgrid[0:H, 0:W].astype(np.float64)
    d = np.stack([(px - K[0, 2]) / K[0, 0], -(py - K[1, 2]) / K[1, 1], -np.ones_like(px)], -1)
    return c2w[:, 3], d @ c2w[:, :3].T


def _sphere_hits(o, d, centre, radius):
    """(hit [H, W], t_in, t_out) of the rays o + t d with the sphere."""
    oc = o - centre
    a, b, c = (d * d).sum(-1), (d * oc).sum(-1), (oc * oc).sum() - radius * radius
    disc = b * b - a * c
    hit = disc > 0
    r = np.sqrt(np.where(hit, disc, 0.0))
    return hit, (-b - r) / a, (-b + r) / a


def _segment_distance(p, a, b):
    ab = b - a
    t = np.clip(((p - a) * ab).sum(1) / np.maximum((ab * ab).sum(1), 1e-300), 0.0, 1.0)
    return np.linalg.norm(a + t[:, None] * ab - p, axis=1)


def _triangle_distance(p, a, b, c):
    """The distance of the point p from each triangle (a, b, c) [n, 3]: to the plane where p projects into the triangle, else to
    the nearest edge."""
    n = np.cross(b - a, c - a)
    nn = np.linalg.norm(n, axis=1)
    inside = nn > 0
    for u, w in ((a, b), (b, c), (c, a)):
        inside &= (np.cross(w - u, p - u) * n).sum(1) >= 0
    plane = np.abs(((p - a) * n).sum(1)) / np.where(nn > 0, nn, 1.0)
    edges = np.minimum(np.minimum(_segment_distance(p, a, b), _segment_distance(p, b, c)), _segment_distance(p, c, a))
    return np.where(inside, plane, edges)


@pytest.mark.parametrize("pose", [0, 1])
@pytest.mark.parametrize("name,H,W", [("tetrahedron", 48, 64), ("sphere12", 48, 64), ("sphere24", 96, 96)])
def test_the_picture_is_watertight(name, H, W, pose):
    """The ball about an interior point that touches no face lies inside the closed mesh, and the mesh inside the ball through its
    farthest vertex.  (For the tetrahedron the inner ball is the sphere inscribed in its face planes.  The planes of the rough
    spheres' faces pass as close as 0.003 to the centre, so there the ball is bounded by the faces themselves, by the exact
    distance from the centre to each triangle.)  A pixel whose centre ray hits the inner ball (shrunk by 1 %: the corners move by
    up to 1 / 512 pixel when they are snapped) is covered; one whose ray misses the outer ball (grown by 1 %) is empty; a covered
    depth lies between the entry into the outer ball and the entry into the inner one, or the exit from the outer one where the
    ray misses the inner one."""
    v, f = MESHES[name]()
    v64 = v.astype(np.float64)
    centre = v64[f].mean((0, 1))
    dist = _triangle_distance(centre, *(v64[f[:, k]] for k in range(3)))
    if name == "tetrahedron":
        a, b, c = (v64[f[:, k]] for k in range(3))
        nrm = np.cross(b - a, c - a)
        plane = ((a - centre) * nrm).sum(1) / np.linalg.norm(nrm, axis=1)
        assert plane.min() > 0 and abs(plane.min() - dist.min()) < 1e-12      # outward faces; the ball touches a face plane
    assert dist.min() > 0.2
    r_in, r_out = 0.99 * dist.min(), 1.01 * np.linalg.norm(v64 - centre, axis=1).max()
    K = R.intrinsics(H, W)
    _, _, face, _, depth, acc = R.render(v, f, R.view_of(POSES[pose], K), H, W, NEAR)
    o, d = _rays(POSES[pose], K, H, W)
    hit_in, t_in, _ = _sphere_hits(o, d, centre, r_in)
    hit_out, t0, t1 = _sphere_hits(o, d, centre, r_out)
    cov = acc.reshape(H, W) == 1.0
    assert hit_in.sum() > 20 and (~hit_out).sum() > 20 and (hit_out & ~hit_in).sum() > 20
    assert cov[hit_in].all() and not cov[~hit_out].any()
    z = depth.reshape(H, W).astype(np.float64)
    assert (z[cov] >= t0[cov] - 1e-4).all() and (z[cov] <= np.where(hit_in, t_in, t1)[cov] + 1e-4).all()
    assert ((face >= 0) == cov.reshape(-1)).all() and not z[~cov].any()


@pytest.mark.parametrize("name", ["sphere12", "sphere24"])
def test_face_order_does_not_change_the_picture(name):
    H, W = 48, 64
    v, f = MESHES[name]()
    view = R.view_of(POSES[1], R.intrinsics(H, W))
    keys, stats, face, bary, depth, acc = R.render(v, f, view, H, W, NEAR)
    perm = np.random.default_rng(7).permutation(len(f))
    k2, s2, face2, _, depth2, acc2 = R.render(v, f[perm], view, H, W, NEAR)
    assert np.array_equal(depth2.view(np.int32), depth.view(np.int32)) and np.array_equal(acc2, acc) and np.array_equal(s2, stats)
    assert np.array_equal(k2 >> np.uint64(32), keys >> np.uint64(32))
    why, X, Y, z, s = R.setup(v, f, view, NEAR)
    ties = np.zeros((H, W), np.int64)
    py, px = np.mgrid[0:H, 0:W]
    for j in np.nonzero(why == R.OK)[0]:
        cov, _, _, d = R.pixel(X[j], Y[j], z[j], s[j], px, py)
        ties += cov & (d.view(np.int32) == depth.view(np.int32).reshape(H, W))
    unique = (face >= 0) & (ties.reshape(-1) == 1)
    assert unique.sum() > 0.9 * (face >= 0).sum() and np.array_equal(perm[face2[unique]], face[unique])
    # where faces tie, the lower index of the order at hand wins: the winner is among the tied faces, and no tied face has a lower one
    inv = np.argsort(perm)
    for p in np.nonzero((face >= 0) & ~unique)[0][:50]:
        tied = [j for j in np.nonzero(why == R.OK)[0]
                if (lambda r: r[0] and r[3].view(np.int32) == depth.view(np.int32)[p])(R.pixel(X[j], Y[j], z[j], s[j], p % W, p // W))]
        assert face[p] == min(tied) and perm[face2[p]] in tied and face2[p] == min(inv[tied])


def test_interpolation_is_perspective_correct():
    """A tilted planar quad (depth 2.2 to 4.4 across the image).  At a covered pixel the rule gives exactly the perspective-correct
    weights of the SNAPPED triangle, whose corners sit within 1 / 512 pixel per axis of the true ones (plus 2^-16 pixel of float32
    rounding in u and v at |u|, |v| < 128), with the true depths.  Those weights are the exact weights of the true triangle at a
    screen point within d = 1 / 512 + 2^-16 pixel per axis of the pixel centre (a convex combination of the corner shifts), so the
    reconstructed point is the plane's point under such a screen point, up to float32 rounding: seven roundings of quantities
    below 8 for the weights and the sum, 8 * 7 * 2^-24 < 4e-6.  The plane's point X(u, v) is a projective function of the
    screen point, monotone along each axis over a pixel here, so over the square of half-side d it deviates from X(centre) by at
    most the largest deviation at the square's corners times (1 + 1 / 16) for its curvature.  The bound is that, evaluated per
    pixel, plus 4e-6; z likewise with the points' depths."""
    H, W = 48, 64
    c2w, K = POSES[0], R.intrinsics(H, W)
    cam = [(-0.9, -0.6, 2.2), (1.7, -0.7, 4.4), (1.6, 0.9, 4.2), (-0.8, 0.5, None)]
    # make it planar in camera space: the fourth corner's depth from the plane of the first three
    p0, p1, p2 = (np.array([x, y, -z]) for x, y, z in cam[:3])
    nrm = np.cross(p1 - p0, p2 - p0)
    x3, y3 = cam[3][0], cam[3][1]
    z3 = -(p0 @ nrm - nrm[0] * x3 - nrm[1] * y3) / nrm[2]
    assert 2.0 < z3 < 3.0
    pts = [R.from_camera(c2w, x, y, z) for x, y, z in cam[:3] + [(x3, y3, z3)]]
    v = np.array(pts, np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    view = R.view_of(c2w, K)
    _, stats, face, bary, depth, acc = R.render(v, f, view, H, W, NEAR)
    cov = face >= 0
    assert stats[0] == 2 and 300 < cov.sum() < H * W
    v64 = v.astype(np.float64)
    A, B, Cc = (v64[f[face[cov], k]] for k in range(3))
    wb, wc = bary[cov, 0].astype(np.float64)[:, None], bary[cov, 1].astype(np.float64)[:, None]
    got = ((1.0 - wb - wc) * A + wb * B) + wc * Cc
    # the analytic ray-plane intersection, with the float32 corners' own plane
    wn = np.cross(v64[1] - v64[0], v64[2] - v64[0])
    o = c2w[:, 3]

    def plane_point(u, w):
        dcam = np.stack([(u - K[0, 2]) / K[0, 0], -(w - K[1, 2]) / K[1, 1], -np.ones_like(u)], -1)
        d = dcam @ c2w[:, :3].T
        t = ((v64[0] - o) @ wn) / (d @ wn)
        return o + t[:, None] * d, t

    py, px = np.divmod(np.nonzero(cov)[0], W)
    want, tz = plane_point(px.astype(np.float64), py.astype(np.float64))
    step = 1.0 / 512 + 2.0 ** -16
    dev_p, dev_z = np.zeros(len(px)), np.zeros(len(px))
    for du in (-step, step):
        for dw in (-step, step):
            q, t = plane_point(px + du, py + dw)
            dev_p = np.maximum(dev_p, np.linalg.norm(q - want, axis=1))
            dev_z = np.maximum(dev_z, np.abs(t - tz))
    err_p, err_z = np.linalg.norm(got - want, axis=1), np.abs(depth[cov].astype(np.float64) - tz)
    print("max point error", err_p.max(), "bound there", (dev_p * (1 + 1 / 16) + 4e-6)[err_p.argmax()], "max z error", err_z.max())
    assert (err_p <= dev_p * (1 + 1 / 16) + 4e-6).all() and (err_z <= dev_z * (1 + 1 / 16) + 4e-6).all()
    assert tz.max() - tz.min() > 1.5                                     # the tilt is real: an affine (screen-space) z would be far off
    u, w, zc = R.project(v, view)
    mid = 0.5 * (zc[0] + zc[1])
    t = plane_point(np.array([0.5 * (u[0] + u[1])], np.float64), np.array([0.5 * (w[0] + w[1])], np.float64))[1][0]
    assert abs(mid - t) > 0.1                                            # (the screen-space midpoint is not at the mean depth)


def test_hidden_surfaces_and_the_tie_rule():
    H, W = 32, 40
    c2w, K = R.look_at([0.0, 0.0, 0.0], [0.0, 0.0, -1.0]), R.intrinsics(H, W)
    view = R.view_of(c2w, K)
    near_q = R.quad(c2w, K, [(4.3, 3.4), (25.6, 3.4), (25.6, 20.7), (4.3, 20.7)], [2.0] * 4)
    far_q = R.quad(c2w, K, [(12.2, 9.1), (36.5, 9.1), (36.5, 28.8), (12.2, 28.8)], [3.0] * 4)
    for order in (0, 1):                                                  # the nearer quad first, and last
        qs = (near_q, far_q) if order == 0 else (far_q, near_q)
        v = np.concatenate([qs[0][0], qs[1][0]])
        f = np.concatenate([qs[0][1], qs[1][1] + 4])
        _, stats, face, _, depth, acc = R.render(v, f, view, H, W, NEAR)
        face, depth = face.reshape(H, W), depth.reshape(H, W)
        near_ids = (0, 1) if order == 0 else (2, 3)
        both = np.zeros((H, W), bool)
        both[10:21, 13:26] = True                                         # the pixels inside both quads
        assert np.isin(face[both], near_ids).all() and np.abs(depth[both] - 2.0).max() < 1e-5
        only_far = np.zeros((H, W), bool)
        only_far[21:29, 13:37] = True
        assert np.isin(face[only_far], (2, 3) if order == 0 else (0, 1)).all() and np.abs(depth[only_far] - 3.0).max() < 1e-5
        assert stats[3] >= acc.sum() + both.sum()                        # every doubly covered pixel got two key updates
    # a square whose corners are pixel centres: the diagonal runs through pixel centres, both triangles cover them at the same
    # depth bits, and the lower index wins whichever triangle it is
    sq, tri = R.quad(c2w, K, [(4, 4), (20, 4), (20, 20), (4, 20)], [2.0] * 4)
    why, X, Y, _, _ = R.setup(sq, tri, view, NEAR)
    assert (X == np.array([[4, 20, 20], [4, 20, 4]]) * 256).all() and (Y == np.array([[4, 4, 20], [4, 20, 20]]) * 256).all()
    diag = np.arange(4, 21)
    for faces in (tri, tri[::-1].copy()):
        _, stats, face, _, _, acc = R.render(sq, faces, view, H, W, NEAR)
        face = face.reshape(H, W)
        assert acc.sum() == 17 * 17 and stats[3] == 17 * 17 + 17         # inclusive edges: the diagonal belongs to both
        assert (face[diag, diag] == 0).all() and (face[4:21, 4:21] >= 0).all() and {0, 1} == set(face[4:21, 4:21].ravel())


def test_dropped_faces_are_counted_where_the_rule_says():
    H, W = 48, 64
    c2w = POSES[0]
    view = R.view_of(c2w, R.intrinsics(H, W))
    v0, f0 = S.sphere(12)
    near = 0.25
    v, f, n_depth, n_other = R.drop_scene(c2w, v0, f0[:101], near)
    assert f.dtype == np.int32 and f.min() == -2 ** 31 and f.max() == 2 ** 31 - 1 and len(v) in f
    assert (R.setup(v0, f0[:101], view, near)[0] == R.OK).all()
    why = R.setup(v, f, view, near)[0]
    assert list(why[[1, 3, 5]]) == [R.DROP_DEPTH] * 3 and list(why[[7, 9, 11, 13, 15, 17, 100]]) == [R.DROP_OTHER] * 7
    keys, stats, face, _, depth, _ = R.render(v, f, view, H, W, near)
    assert list(stats[:3]) == [101 - n_depth - n_other, n_depth, n_other] and stats[3] > 0
    assert not np.isin(face, [1, 3, 5, 7, 9, 11, 13, 15, 17, 100]).any() and (face >= 0).sum() > 50
    assert np.isfinite(depth).all() and (depth[face >= 0] >= near).all()
    # a face wholly in front of near, and everything once near lies behind the mesh
    assert list(R.render(v0, f0[:101], view, H, W, 10.0)[1]) == [0, 101, 0, 0]
    # an index is never read through: no vertices at all
    assert list(R.render(np.zeros((0, 3), np.float32), f0[:5], view, H, W, near)[1]) == [0, 0, 5, 0]


@pytest.mark.parametrize("name", ["sphere12", "sphere24"])
def test_culling_halves_a_closed_surface_and_changes_no_pixel(name):
    H, W = 48, 64
    v, f = MESHES[name]()
    view = R.view_of(POSES[0], R.intrinsics(H, W))
    plain, culled = R.render(v, f, view, H, W, NEAR), R.render(v, f, view, H, W, NEAR, cull=True)
    for a, b in zip(plain[2:], culled[2:]):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    assert np.array_equal(plain[0], culled[0])
    s0, s1 = plain[1], culled[1]
    assert s1[0] + s1[2] == s0[0] + s0[2] and s1[1] == s0[1] == 0
    # seen from outside, every ray enters a closed surface as often as it leaves it: half of the (pixel, face) pairs are front faces
    assert 2 * s1[3] == s0[3] and 0.25 * s0[0] < s1[0] < 0.75 * s0[0]
