"""The projective texture bake without a GPU: the header / binding / Makefile / engine / trainer / tool bookkeeping, the argument
checks of the C ABI (they return before any device work, so they run here; and once more in a stand-alone program under
-fsanitize=address,undefined, tests/project_check.cpp) and of engine.mesh, and the properties of the rule of include/nerf_hip.h
"view-projected texture" on its numpy statement tests/_project_ref.py: constant images, an affine image, occlusion, back-facing
and grazing texels, and the order of the views.  The kernels are held to that reference bit for bit in tests/test_gpu_project.py."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import _project_ref as P
from tests import _raster_ref as R
from tests import _smooth_ref as S
from tests import _texture_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE = -1, -2
ENTRIES = ["nerf_project_accumulate", "nerf_project_finish"]
KERNELS = ["project_accumulate_kernel", "project_finish_kernel"]
NEAR = 0.01
F32 = np.float32


def _lib():
    from nerf_meets_mlx_amd import _native
    return _native.lib()


# ------------------------------------------------------------------------------------------------ bookkeeping
def test_header_section_bindings_and_makefile():
    from nerf_meets_mlx_amd import _native
    from nerf_meets_mlx_amd.engine import mesh as E
    text = open(os.path.join(ROOT, "include", "nerf_hip.h")).read()
    start = text.index("/* ---------------------------------------------------------------- view-projected texture (no reference counterpart)")
    banners = [m.start() for m in re.finditer(r"/\* ----", text)]
    k = banners.index(start)
    assert text[banners[k - 1]:].startswith("/* ---------------------------------------------------------------- fused renderer (a14 / a18)")
    section = text[start:banners[k + 1]]
    decl = re.sub(r"/\*.*?\*/", "", section, flags=re.S)
    assert sorted(set(re.findall(r"\b(nerf_project_[a-z_]+)\s*\(", decl))) == ENTRIES
    assert sorted(set(re.findall(r"\b(nerf_project_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))) == ENTRIES
    assert f"#define NERF_PROJECT_MAX_VIEWS {E.PROJECT_MAX_VIEWS}" in decl and P.MAX_VIEWS == E.PROJECT_MAX_VIEWS == 16
    assert "#define NERF_PROJECT_BLEND 0" in decl and "#define NERF_PROJECT_BEST 1" in decl
    assert E.PROJECT_MODES == {"blend": P.BLEND, "best": P.BEST} == P.MODES
    assert "#define NERF_ABI_VERSION 3" in text
    lib = _lib()
    assert lib.nerf_abi_version() == 3
    for e in ENTRIES:
        assert e in _native.SIGNATURES and hasattr(lib, e)
    assert sorted(s for s in _native.SIGNATURES if s.startswith("nerf_project_")) == ENTRIES
    for word in ("zc = 0.0f - z_w", "cosv = ((n0 e0 + n1 e1) + n2 e2) / L", "floorf(u + 0.5f)", "ez = s / a - zc",
                 "((w00 c00 + w10 c10) + w01 c01) + w11 c11", "w > S_w", "Not done", "alpha-weighted", "mipmaps", "seam levelling",
                 "exposure", "clipping"):
        assert word in section, word
    mk = open(os.path.join(ROOT, "nerf_meets_mlx_amd", "csrc", "Makefile")).read()
    assert "project.hip" in next(ln for ln in mk.splitlines() if ln.startswith("SRCS")).split()
    assert "project.h" in next(ln for ln in mk.splitlines() if ln.startswith("HDRS")).split()
    src = open(os.path.join(ROOT, "nerf_meets_mlx_amd", "csrc", "project.hip")).read()
    assert sorted(set(re.findall(r"\b(\w+_kernel)\(", src))) == KERNELS
    code = re.sub(r"//.*", "", src + open(os.path.join(ROOT, "nerf_meets_mlx_amd", "csrc", "project.h")).read())
    assert "atomic" not in code
    # the texel is texture.hip's through texture.h, not a copy
    assert "tex_point(" in code and "tex_texel(" in code and "sqrt_rn((m[0]" not in code


def test_signatures_and_defaults():
    from nerf_meets_mlx_amd.engine import mesh as E
    from nerf_meets_mlx_amd.engine.ngp import NGPTrainer
    from nerf_meets_mlx_amd.engine.trainer import Trainer
    p = inspect.signature(E.project_texture).parameters
    assert list(p) == ["mesh", "images", "c2w", "K", "texels", "depth_tol", "mode", "fallback", "depth", "acc", "near", "cos_min",
                       "acc_min", "chunk", "mark"]
    assert [p[k].default for k in list(p)[4:]] == [8, None, "blend", None, None, None, E.RASTER_NEAR, E.PROJECT_COS_MIN, 0.5, E.CHUNK, None]
    p = inspect.signature(Trainer.project_texture).parameters
    assert list(p) == ["self", "mesh", "texels", "views", "source", "mode", "fallback", "depth_tol"]
    assert [p[k].default for k in list(p)[2:]] == [8, None, "images", "blend", True, None]
    assert NGPTrainer.project_texture is Trainer.project_texture
    assert 0.0 < E.PROJECT_COS_MIN <= 1.0 and E.PROJECT_DEPTH_TOL_CELLS > 0.0
    # what was there before is what it was
    assert E.Mesh._fields == ("verts", "faces", "normals", "colors") and E.Texture._fields == ("image", "uv", "texels")
    assert E.MeshFrame._fields == ("rgb", "depth", "acc", "face", "bary")
    assert list(inspect.signature(E.bake_texture).parameters) == ["query", "mesh", "texels", "chunk", "mark"]
    assert list(inspect.signature(E.sample_texture).parameters) == ["texture", "mesh", "face", "bary", "rows"]
    assert list(inspect.signature(E.rasterize).parameters) == ["mesh", "c2w", "K", "H", "W", "near", "cull_backfaces", "mark", "small_max"]
    assert list(inspect.signature(E.render_mesh).parameters) == ["mesh", "c2w", "K", "H", "W", "texture", "background", "near",
                                                                 "cull_backfaces", "mark", "small_max"]
    assert list(inspect.signature(E.write_obj).parameters) == ["path", "mesh", "texture"]
    assert list(inspect.signature(Trainer.texture_mesh).parameters) == ["self", "mesh", "texels"]
    assert list(inspect.signature(Trainer.render_mesh).parameters) == ["self", "mesh", "c2w", "texture", "background"]


def test_mesh_tool_knows_the_project_kernels_and_flag(tmp_path, capsys):
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
    assert tool.parser().parse_args(["--project"]).project and not tool.parser().parse_args([]).project
    # state read and written, and per view two map reads and four corners of three floats; state read, four bytes written
    assert tool._project_bytes("project_accumulate_kernel", 1000, 16) == 1000 * (32 + 16 * 56)
    assert tool._project_bytes("project_finish_kernel", 1000, 16) == 1000 * 20


# ------------------------------------------------------------------------------------------------ argument errors
def test_every_argument_error_returns_before_device_work():
    """Without a device the first launch would fail with NERF_E_HIP: every refusal below is NERF_E_SHAPE or NERF_E_NULL, so it was
    made before any device work.  The device pointers are never dereferenced."""
    lib = _lib()
    p = C.c_void_p(4096)
    big = (1 << 24) + 1
    good = np.stack([R.view_of(R.look_at(S.CENTRE + [2.6, 1.1, 2.2], S.CENTRE), R.intrinsics(48, 64))] * 16)

    def acc(verts=p, normals=p, V=10, faces=p, F=9, T_=8, p0=0, count=5, views=good, n=2, H=48, W=64, images=p, depth=p, acc_=p, near=0.5,
            tol=0.01, cos_min=0.1, acc_min=0.5, mode=0, state=p):
        v = None if views is None else np.ascontiguousarray(views, np.float32).ctypes.data_as(C.POINTER(C.c_float))
        return lib.nerf_project_accumulate(verts, normals, V, faces, F, T_, p0, count, v, n, H, W, images, depth, acc_, near, tol, cos_min,
                                           acc_min, mode, state, None)

    def fin(state=p, F=9, T_=8, p0=0, count=5, mode=1, fallback=None, image=p, seen=p):
        return lib.nerf_project_finish(state, F, T_, p0, count, mode, fallback, image, seen, None)

    def bad_views(s, q, value):
        v = good.copy()
        v[s, q] = value
        return v

    assert T.layout(9, 8) == (30, 20, 3, 10)
    Pn = 30 * 20
    nan, inf = float("nan"), float("inf")
    shape = {"nerf_project_accumulate": [{"n": -1}, {"n": 17}, {"H": 0}, {"W": 0}, {"H": 16385}, {"W": 16385}, {"H": -1}, {"T_": 1},
                                         {"T_": 65}, {"F": -1}, {"F": big}, {"F": 1 << 24}, {"V": -1}, {"V": big}, {"near": 0.0},
                                         {"near": -1.0}, {"near": inf}, {"near": nan}, {"tol": -1e-3}, {"tol": inf}, {"tol": nan},
                                         {"cos_min": 0.0}, {"cos_min": 1.5}, {"cos_min": nan}, {"cos_min": -0.1}, {"acc_min": 0.0},
                                         {"acc_min": 1.001}, {"acc_min": nan}, {"mode": 2}, {"mode": -1}, {"p0": -1}, {"count": -1},
                                         {"p0": Pn - 4}, {"p0": Pn, "count": 1}, {"count": Pn + 1}, {"p0": 1 << 62, "count": 1 << 62},
                                         {"state": C.c_void_p(4100)}]
             + [{"views": bad_views(1, q, nan)} for q in range(16)] + [{"views": bad_views(0, 12, inf)},
                                                                        {"views": bad_views(15, 3, -inf), "n": 16}],
             "nerf_project_finish": [{"T_": 1}, {"T_": 65}, {"F": -1}, {"F": big}, {"F": 1 << 24}, {"mode": 2}, {"mode": -1}, {"p0": -1},
                                     {"count": -1}, {"p0": Pn, "count": 1}, {"count": Pn + 1}, {"state": C.c_void_p(4104)}]}
    null = {"nerf_project_accumulate": [{"views": None}, {"verts": None}, {"normals": None}, {"faces": None}, {"images": None},
                                        {"depth": None}, {"acc_": None}, {"state": None}],
            "nerf_project_finish": [{"state": None}, {"image": None}, {"seen": None}]}
    call = {"nerf_project_accumulate": acc, "nerf_project_finish": fin}
    for want, table in ((E_SHAPE, shape), (E_NULL, null)):
        for name, cases in table.items():
            for kw in cases:
                assert call[name](**kw) == want, (name, {k: v for k, v in kw.items() if k != "views"})
                assert name.encode() in lib.nerf_last_error(), (name, kw, lib.nerf_last_error())
    # a non-finite number in a view past the n-th is not looked at; nothing to do is no error and needs neither pointers nor a device
    assert acc(n=0, views=None, images=None, depth=None, acc_=None, state=None) == 0
    assert acc(count=0, state=None, images=None) == 0 and acc(p0=Pn, count=0) == 0 and acc(n=0, views=bad_views(0, 0, nan)) == 0
    assert acc(count=0, views=bad_views(2, 0, nan)) == 0 and acc(count=0, state=C.c_void_p(4100)) == 0
    assert fin(count=0, state=None, image=None, seen=None) == 0 and fin(p0=Pn, count=0) == 0


def test_argument_checks_under_sanitizers(tmp_path):
    """csrc/project.h's two check functions, all the host code of the two entries ahead of their launch, in a stand-alone program
    built with the host compiler and -fsanitize=address,undefined (tests/project_check.cpp)."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "project_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "project_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    want = {"ok": (0, 1), "idle": (0, 0), "shape": (E_SHAPE, 0), "null": (E_NULL, 0)}
    seen = {k: 0 for k in want}
    for ln in out.stdout.splitlines():
        name, rc, work, copied = ln.split()
        kind = name.split(".")[0]
        assert (int(rc), int(work)) == want[kind] and int(copied) == 1, ln
        seen[kind] += 1
    assert seen["ok"] >= 8 and seen["idle"] >= 4 and seen["shape"] >= 55 and seen["null"] >= 11


def test_engine_argument_checks():
    from nerf_meets_mlx_amd.engine import mesh as E
    v, f = (torch.from_numpy(a.copy()) for a in S.sphere(12))
    good = E.Mesh(v, f, torch.zeros_like(v), None)
    assert E.check_project_args(0.02) == (0.02, 0, E.RASTER_NEAR, E.PROJECT_COS_MIN, 0.5, E.CHUNK)
    assert E.check_project_args(0, "best", 2, 1, 1.0, np.int64(7)) == (0.0, 1, 2.0, 1.0, 1.0, 7)
    for kw in ({"depth_tol": None}, {"depth_tol": -1e-3}, {"depth_tol": float("nan")}, {"depth_tol": float("inf")}, {"depth_tol": True},
               {"depth_tol": "0.1"}, {"depth_tol": 1e39}, {"mode": "mean"}, {"mode": 0}, {"mode": None}, {"near": 0.0}, {"near": float("inf")},
               {"near": None}, {"cos_min": 0.0}, {"cos_min": 1.5}, {"cos_min": float("nan")}, {"cos_min": None}, {"cos_min": 1e-60},
               {"acc_min": 0.0}, {"acc_min": 1.01}, {"acc_min": True}, {"chunk": 0}, {"chunk": 2.0}, {"chunk": True}):
        args = {"depth_tol": 0.02, **kw}
        with pytest.raises(ValueError, match="project " + next(iter(kw)) if "near" not in kw else "near"):
            E.check_project_args(**args)
    K, pose = R.intrinsics(6, 8), R.look_at(S.CENTRE + [2.6, 1.1, 2.2], S.CENTRE)
    images, poses = torch.zeros(2, 6, 8, 3), np.stack([pose, pose])
    tex = E.Texture(torch.zeros(T.layout(len(f), 2)[1], T.layout(len(f), 2)[0], 3, dtype=torch.uint8), torch.zeros(len(f), 3, 2), 2)
    maps = torch.zeros(2, 6, 8)
    bad = [dict(images=images.double()), dict(images=images[..., :2]), dict(images=torch.zeros(2, 6, 8, 4)), dict(images=images[0]),
           dict(images=images.numpy()), dict(images=images.permute(0, 2, 1, 3)), dict(c2w=poses[:1]), dict(c2w=np.zeros((2, 2, 4))),
           dict(K=np.eye(4)), dict(texels=1), dict(texels=2.0), dict(depth_tol=None), dict(depth_tol=-1.0), dict(mode="max"),
           dict(fallback=tex._replace(texels=3)), dict(fallback=tex.image), dict(fallback=tex._replace(image=tex.image[:-1])),
           dict(texels=3, fallback=tex), dict(depth=maps), dict(acc=maps), dict(depth=maps[:1], acc=maps), dict(depth=maps.double(), acc=maps),
           dict(depth=maps, acc=maps.numpy()), dict(near=0.0), dict(cos_min=0.0), dict(acc_min=2.0), dict(chunk=0),
           dict(mesh=good._replace(normals=None)), dict(mesh=good._replace(faces=f.long())), dict(mesh=(v, f))]
    for kw in bad:
        args = dict(mesh=good, images=images, c2w=poses, K=K, texels=2, depth_tol=0.02)
        args.update(kw)
        with pytest.raises(ValueError):
            E.project_texture(**args)
    with pytest.raises(ValueError, match="RGBA"):
        E.project_texture(good, torch.zeros(2, 6, 8, 4), poses, K, 2, 0.02)
    # an image larger than the rasteriser takes is refused by its size alone, ahead of anything else
    with pytest.raises(ValueError, match="16384"):
        E.project_texture(good, torch.zeros(1, 1, 16385, 3), poses[:1], K, 2, 0.02)


def test_no_faces_and_no_views_launch_nothing():
    """F = 0: a black cell (or the fallback's), nothing seen, and no device is needed; n = 0 with F = 0 likewise."""
    from nerf_meets_mlx_amd.engine import mesh as E
    v = torch.from_numpy(S.tetrahedron()[0].copy())
    m = E.Mesh(v, torch.zeros(0, 3, dtype=torch.int32), torch.zeros_like(v))
    K, pose = R.intrinsics(6, 8), R.look_at(S.CENTRE + [2.6, 1.1, 2.2], S.CENTRE)
    for images, poses in ((torch.rand(2, 6, 8, 3), np.stack([pose, pose])), (torch.zeros(0, 6, 8, 3), np.zeros((0, 3, 4)))):
        tex, seen = E.project_texture(m, images, poses, K, 6, 0.02)
        assert tex.image.shape == (8, 8, 3) and tex.image.dtype == torch.uint8 and not tex.image.any()
        assert seen.shape == (8, 8) and seen.dtype == torch.uint8 and not seen.any()
        assert tex.uv.shape == (0, 3, 2) and tex.texels == 6
    fb = E.Texture(torch.full((8, 8, 3), 7, dtype=torch.uint8), torch.zeros(0, 3, 2), 6)
    tex, seen = E.project_texture(m, torch.rand(1, 6, 8, 3), pose, K, 6, 0.02, fallback=fb)
    assert bool((tex.image == 7).all()) and not seen.any() and tex.image.data_ptr() != fb.image.data_ptr()


def test_trainer_argument_checks():
    """The refusals Trainer.project_texture makes itself come before any device work: a stand-in with the attributes they read."""
    from nerf_meets_mlx_amd.engine.trainer import Trainer

    class Stub:
        poses = torch.zeros(4, 4, 4)
        images = torch.zeros(4, 6, 8, 4)
        _mesh_box = Trainer._mesh_box

    stub = Stub()
    with pytest.raises(ValueError, match='source="field"'):
        Trainer.project_texture(stub, None)
    with pytest.raises(ValueError, match="source must be"):
        Trainer.project_texture(stub, None, source="frames")
    for views in ([4], [-1], [0, 9]):
        with pytest.raises(ValueError, match="views"):
            Trainer.project_texture(stub, None, views=views, source="field")
    stub.images = torch.zeros(4, 6, 8, 3)
    with pytest.raises(ValueError, match="pass depth_tol"):
        Trainer.project_texture(stub, None)


# ------------------------------------------------------------------------------------------------ the rule, on the reference
POSES = [R.look_at(S.CENTRE + [2.6, 1.1, 2.2], S.CENTRE), R.look_at(S.CENTRE + [-2.0, -0.7, 2.4], S.CENTRE),
         R.look_at(S.CENTRE + [0.3, 2.9, -1.0], S.CENTRE)]
TOL, COS_MIN = 0.05, 0.1


@pytest.fixture(scope="module")
def sphere():
    """sphere24 seen by three cameras at 96 x 96: the mesh, its texels and the maps, computed once."""
    v, f = S.sphere(24)
    nrm = T.vertex_normals(v, f)
    H = W = 96
    K = R.intrinsics(H, W)
    views = np.stack([R.view_of(p, K) for p in POSES])
    both = [P.maps(v, f, vw, H, W, NEAR) for vw in views]
    return {"v": v, "f": f, "n": nrm, "H": H, "W": W, "views": views, "depth": np.stack([b[0] for b in both]),
            "acc": np.stack([b[1] for b in both]), "texels": P.texels(v, nrm, f, 8), "lay": T.layout(len(f), 8)}


def _bake(s, images, mode, order=None, fallback=None, cos_min=COS_MIN):
    k = list(range(len(images))) if order is None else list(order)
    return P.bake(s["v"], s["n"], s["f"], 8, s["views"][k], np.asarray(images, F32)[k], NEAR, TOL, cos_min, 0.5, mode, fallback,
                  s["depth"][k], s["acc"][k])


def _seen_by(s, k, cos_min=COS_MIN):
    ok, x, n = s["texels"]
    img = np.zeros((s["H"], s["W"], 3), F32)
    return P.observe(s["views"][k], img, s["depth"][k], s["acc"][k], x, n, NEAR, TOL, cos_min, 0.5)[0] & ok


def test_constant_images(sphere):
    s = sphere
    H, W = s["H"], s["W"]
    images = np.zeros((2, H, W, 3), F32)
    images[0, ..., 0], images[1, ..., 1] = 1.0, 1.0
    fallback = np.random.default_rng(3).integers(0, 256, (s["lay"][1], s["lay"][0], 3)).astype(np.uint8)
    a, b = _seen_by(s, 0), _seen_by(s, 1)
    assert (a & ~b).sum() > 500 and (b & ~a).sum() > 500 and (a & b).sum() > 200 and (~a & ~b).sum() > 500
    for mode in (P.BLEND, P.BEST):
        image, seen, _ = _bake(s, images, mode, fallback=fallback)
        px = image.reshape(-1, 3).astype(np.int64)
        assert np.array_equal(seen.reshape(-1) == 1, a | b)
        assert (px[a & ~b] == [255, 0, 0]).all() and (px[b & ~a] == [0, 255, 0]).all()
        assert np.array_equal(px[~a & ~b], fallback.reshape(-1, 3)[~a & ~b])
        both = px[a & b]
        if mode == P.BLEND:
            assert (both[:, 2] == 0).all() and (np.abs(both[:, 0] + both[:, 1] - 255) <= 1).all()
            assert (both[:, 0] > 0).all() and (both[:, 1] > 0).all()
        else:
            red, green = (both == [255, 0, 0]).all(1), (both == [0, 255, 0]).all(1)
            assert (red | green).all() and red.any() and green.any()
    # without a fallback the unseen texels are black
    assert not _bake(s, images, P.BLEND)[0].reshape(-1, 3)[~a & ~b].any()


def test_affine_image_is_reproduced_at_the_texels_own_projection(sphere):
    """Bilinear interpolation reproduces a function that is affine in pixel coordinates: every seen texel's byte lies within half
    a byte step (0.5 / 255) and float32 rounding (1e-5) of the function at the texel's own (u, v), recomputed in float64."""
    s = sphere
    H, W = s["H"], s["W"]
    py, px = np.mgrid[0:H, 0:W].astype(np.float64)
    coef = np.array([[0.15, 0.004, 0.003], [0.8, -0.005, 0.001], [0.3, 0.002, -0.0015]])
    image = np.stack([c[0] + c[1] * px + c[2] * py for c in coef], -1)
    assert 0.05 < image.min() and image.max() < 0.95
    out, seen, _ = _bake(s, image[None].astype(F32), P.BLEND, order=[0])
    ok, x, _ = s["texels"]
    got = seen.reshape(-1) == 1
    assert got.sum() > 2000
    c, K = np.asarray(POSES[0], np.float64), R.intrinsics(H, W)
    q = (x[got].astype(np.float64) - c[:, 3]) @ c[:, :3]
    u, v = K[0, 0] * q[:, 0] / -q[:, 2] + K[0, 2], K[1, 2] - K[1, 1] * q[:, 1] / -q[:, 2]
    want = np.stack([k[0] + k[1] * u + k[2] * v for k in coef], -1)
    err = np.abs(out.reshape(-1, 3)[got] / 255.0 - want).max()
    print("affine image: largest error", err)
    assert err <= 0.5 / 255 + 1e-5


def test_occlusion():
    """Two camera-facing quads at depths 2 and 3, the front one smaller, the back one a little larger than the image: what of the
    back quad lies behind the front one's footprint is unseen, what lies outside it and inside the image is seen, what lies outside
    the image is unseen.  The bands of one pixel either side of the footprint's edge and of the image's border, where the
    nearest-pixel depth lookup or the bilinear footprint may go either way, are left out."""
    H = W = 96
    pose, K = R.look_at([0.0, 0.0, 4.0], [0.0, 0.0, 0.0]), R.intrinsics(H, W)
    view = R.view_of(pose, K)
    lo, hi = 33.0, 63.0                                                     # the front quad: 30 x 30 pixels
    fv, ff = R.quad(pose, K, [(lo, lo), (hi, lo), (hi, hi), (lo, hi)], [2.0] * 4)
    bv, bf = R.quad(pose, K, [(-3.0, -3.0), (98.5, -3.0), (98.5, 98.5), (-3.0, 98.5)], [3.0] * 4)
    v, f = np.concatenate([bv, fv]), np.concatenate([bf, ff + 4])           # faces 0, 1: the back quad
    if R.setup(v, f, view, NEAR)[4][0] > 0:                                 # counter-clockwise seen from the camera: front faces
        f = f[:, ::-1].copy()
    nrm = T.vertex_normals(v, f)
    assert (nrm @ pose[:, 2] > 0.99).all()                                  # both quads face the camera
    Tn = 48
    lay = T.layout(len(f), Tn)
    image = np.full((1, H, W, 3), 0.5, F32)
    _, seen, _ = P.bake(v, nrm, f, Tn, view[None], image, NEAR, 0.05, 0.1)
    ok, x, _ = P.texels(v, nrm, f, Tn)
    p = np.arange(lay[0] * lay[1])
    face = T.owner(lay, p % lay[0], p // lay[0])[0]
    back = ok & (face < 2)
    u, w, _ = R.project(x, view)
    inside_front = np.minimum(np.minimum(u - lo, hi - u), np.minimum(w - lo, hi - w))                    # > 0 inside the footprint
    inside_image = np.minimum(np.minimum(u, (W - 1) - u), np.minimum(w, (H - 1) - w))                    # > 0 between the outer centres
    hidden = back & (inside_front > 1)
    clear = back & (inside_front < -1) & (inside_image > 1)
    outside = back & (inside_image < -1)
    band = back & ~hidden & ~clear & ~outside
    print("occlusion: back texels", back.sum(), "hidden", hidden.sum(), "clear", clear.sum(), "outside", outside.sum(), "band", band.sum())
    assert band.sum() <= 0.2 * back.sum() and hidden.sum() > 100 and clear.sum() > 1000 and outside.sum() > 20
    got = seen.reshape(-1) == 1
    assert not got[hidden].any() and got[clear].all() and not got[outside].any()
    assert got[ok & (face >= 2)].sum() > 1000                               # the front quad itself is seen


def test_back_facing_and_grazing_texels_are_not_seen(sphere):
    s = sphere
    ok, x, n = s["texels"]
    for k, pose in enumerate(POSES):
        for cos_min in (0.05, 0.3):
            got = _seen_by(s, k, cos_min)
            e = np.asarray(pose, np.float64)[:, 3] - x.astype(np.float64)
            cosv = (n.astype(np.float64) * e).sum(1) / np.linalg.norm(e, axis=1)
            assert got.sum() > 1000 and not got[cosv < cos_min - 1e-6].any()
            assert not got[~ok].any()
    assert _seen_by(s, 0, 0.05).sum() > _seen_by(s, 0, 0.3).sum()


def test_order_of_the_views(sphere):
    s = sphere
    rng = np.random.default_rng(11)
    images = rng.random((3, s["H"], s["W"], 3)).astype(F32)
    order = [2, 0, 1]
    for mode in (P.BLEND, P.BEST):
        a, seen_a, st_a = _bake(s, images, mode)
        b, seen_b, st_b = _bake(s, images, mode, order=order)
        assert np.array_equal(seen_a, seen_b) and seen_a.sum() > 3000
        diff = np.abs(a.astype(np.int64) - b.astype(np.int64))
        if mode == P.BLEND:
            assert diff.max() <= 1
        else:
            ok, x, n = s["texels"]
            w = np.stack([np.where(g, c, -1.0) for g, c in (P.observe(s["views"][k], images[k], s["depth"][k], s["acc"][k], x, n, NEAR, TOL,
                                                                      COS_MIN, 0.5)[:2] for k in range(3))])
            top = np.sort(w, 0)
            tie = (top[-1] == top[-2]) & (top[-1] > 0)
            print("order: ties", tie.sum())
            assert not diff.reshape(-1, 3)[~tie].any()
            assert np.array_equal(st_a.view(np.int32)[~tie], st_b.view(np.int32)[~tie])
