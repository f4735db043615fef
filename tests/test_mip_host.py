"""The texture mip pyramid without a GPU: the header / binding / Makefile / engine / trainer / tool bookkeeping, nerf_mip_levels, the
argument checks of the C ABI (they return before any device work, so they run here) and of engine.mesh, and the properties of the
rule of include/nerf_hip.h "texture mip pyramid" on its numpy statement tests/_mip_ref.py: constants, no read outside the face,
an affine field, and less aliasing on a checker.  The kernels are held to that reference bit for bit in tests/test_gpu_mip.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import _mip_ref as M
from tests import _raster_ref as R
from tests import _smooth_ref as S
from tests import _texture_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE = -1, -2
ENTRIES = ["nerf_mip_levels", "nerf_mip_lod", "nerf_mip_reduce", "nerf_mip_sample"]
KERNELS = ["mip_lod_kernel", "mip_reduce_kernel", "mip_sample_kernel"]
BANNER = "/* ---------------------------------------------------------------- "
AFFINE_M = np.array([[0.1, 0.05, -0.08], [-0.06, 0.1, 0.07], [0.04, -0.09, 0.1]])       # tests/test_gpu_texture.py's field
AFFINE_C = np.array([0.5, 0.42, 0.3])
F32 = np.float32


def _lib():
    from nerf_meets_mlx_amd import _native
    return _native.lib()


def _tool():
    import importlib.util
    spec = importlib.util.spec_from_file_location("ngp_mesh_tool", os.path.join(ROOT, "tools", "ngp_mesh.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


# ------------------------------------------------------------------------------------------------ bookkeeping
def test_header_section_bindings_and_makefile():
    from nerf_meets_mlx_amd import _native
    from nerf_meets_mlx_amd.engine import mesh as E
    text = open(os.path.join(ROOT, "include", "nerf_hip.h")).read()
    start = text.index(BANNER + "texture mip pyramid (no reference counterpart)")
    banners = [m.start() for m in re.finditer(r"/\* ----", text)]
    k = banners.index(start)
    assert text[banners[k - 1]:].startswith(BANNER + "view-projected texture (no reference counterpart)")
    assert text[banners[k + 1]:].startswith(BANNER + "gradient all-reduce")
    section = text[start:banners[k + 1]]
    decl = re.sub(r"/\*.*?\*/", "", section, flags=re.S)
    assert sorted(set(re.findall(r"\b(nerf_mip_[a-z_]+)\s*\(", decl))) == ENTRIES
    assert sorted(set(re.findall(r"\b(nerf_mip_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))) == ENTRIES
    assert f"#define NERF_MIP_MAX_LEVELS {E.MIP_MAX_LEVELS}" in decl and M.MAX_LEVELS == E.MIP_MAX_LEVELS == 6
    assert "#define NERF_ABI_VERSION 3" in text
    lib = _lib()
    assert lib.nerf_abi_version() == 3
    for e in ENTRIES:
        assert e in _native.SIGNATURES and hasattr(lib, e)
    assert sorted(s for s in _native.SIGNATURES if s.startswith("nerf_mip_")) == ENTRIES
    for word in ("T_{l+1} = (T_l + 1) / 2", "d = 0.25f r", "((p0 + p1) + (p2 + p3)) 0.125f", "g(i, 0) = 2 v(i - 1, 0) - v(i - 2, 0)",
                 "g = scale (sqrt((float)S) / 256.0f)", "((1.0f - t) c_l) + (t c_{l+1})", "Not done", "anisotropic", "per-pixel",
                 "chart packing", "seam levelling", "push-pull", "supersampled", "OBJ"):
        assert word in section, word
    mk = open(os.path.join(ROOT, "nerf_meets_mlx_amd", "csrc", "Makefile")).read()
    assert "mip.hip" in next(ln for ln in mk.splitlines() if ln.startswith("SRCS")).split()
    assert "mip.h" in next(ln for ln in mk.splitlines() if ln.startswith("HDRS")).split()
    csrc = os.path.join(ROOT, "nerf_meets_mlx_amd", "csrc")
    src = open(os.path.join(csrc, "mip.hip")).read()
    assert sorted(set(re.findall(r"\b(\w+_kernel)\(", src))) == KERNELS
    code = re.sub(r"//.*", "", src + open(os.path.join(csrc, "mip.h")).read())
    assert "atomic" not in code
    # the bilinear lookup is texture.h's, used by the sampler of texture.hip and by mip.hip: one copy
    tex = re.sub(r"//.*", "", open(os.path.join(csrc, "texture.hip")).read())
    assert "tex_lookup(" in tex and "tex_lookup(" in code and "255.0f)" not in tex
    assert len(re.findall(r"\btex_lookup\(const", open(os.path.join(csrc, "texture.h")).read())) == 1


def test_signatures_and_defaults():
    from nerf_meets_mlx_amd.engine import mesh as E
    from nerf_meets_mlx_amd.engine.ngp import NGPTrainer
    from nerf_meets_mlx_amd.engine.trainer import Trainer
    assert E.TexturePyramid._fields == ("levels",)
    assert list(inspect.signature(E.mip_levels).parameters) == ["texels"]
    p = inspect.signature(E.build_mipmaps).parameters
    assert list(p) == ["texture", "mesh", "chunk", "mark"] and (p["chunk"].default, p["mark"].default) == (E.CHUNK, None)
    p = inspect.signature(E.face_lod).parameters
    assert list(p) == ["mesh", "c2w", "K", "near", "texels", "scale"]
    assert [p[k].default for k in list(p)[3:]] == [E.RASTER_NEAR, 8, 1.0]
    p = inspect.signature(E.sample_texture_mip).parameters
    assert list(p) == ["pyramid", "mesh", "face", "bary", "lod", "per_face"] and p["per_face"].default is False
    p = inspect.signature(E.render_mesh_mip).parameters
    assert list(p) == ["mesh", "c2w", "K", "H", "W", "pyramid", "background", "near", "cull_backfaces", "mark", "small_max", "lod_scale"]
    assert [p[k].default for k in list(p)[6:]] == [None, E.RASTER_NEAR, False, None, E.RASTER_SMALL_MAX, 1.0]
    assert list(inspect.signature(Trainer.mip_texture).parameters) == ["self", "mesh", "texture"]
    p = inspect.signature(Trainer.render_mesh_mip).parameters
    assert list(p) == ["self", "mesh", "c2w", "pyramid", "background", "lod_scale"]
    assert (p["background"].default, p["lod_scale"].default) == (None, 1.0)
    p = inspect.signature(Trainer.mesh_psnr_mip).parameters
    assert list(p) == ["self", "mesh", "c2w", "gt", "pyramid", "background", "lod_scale"]
    assert (p["background"].default, p["lod_scale"].default) == (None, 1.0)
    for name in ("mip_texture", "render_mesh_mip", "mesh_psnr_mip"):
        assert getattr(NGPTrainer, name) is getattr(Trainer, name)
    # what was there before is what it was
    assert E.Mesh._fields == ("verts", "faces", "normals", "colors") and E.Texture._fields == ("image", "uv", "texels")
    assert E.MeshFrame._fields == ("rgb", "depth", "acc", "face", "bary")
    assert list(inspect.signature(E.render_mesh).parameters) == ["mesh", "c2w", "K", "H", "W", "texture", "background", "near",
                                                                 "cull_backfaces", "mark", "small_max"]
    assert list(inspect.signature(E.write_obj).parameters) == ["path", "mesh", "texture"]


def test_mesh_tool_knows_the_mip_kernels_and_flag(tmp_path, capsys):
    import argparse
    import json
    tool = _tool()
    path = tmp_path / "trace.csv"
    with open(path, "w") as fh:
        fh.write('"Kernel_Name","Start_Timestamp","End_Timestamp","Grid_Size_X"\n')
        for i, k in enumerate(KERNELS):
            for rep in range(2):
                fh.write(f'"nerf::(anonymous namespace)::{k}(float const*, int)",{1000 * i},{1000 * i + 500 + 1000 * rep},{256 * (i + 1)}\n')
    tool.stats(argparse.Namespace(stats=str(path), from_=None, out=None))
    recs = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert sorted(r["kernel"] for r in recs) == KERNELS and all(r["launches"] == 2 and r["avg_us"] == 1.0 for r in recs)
    assert all(r["bytes_per_item"] == tool._mip_bytes(r["kernel"], 1) for r in recs)
    assert tool.parser().parse_args(["--mip"]).mip and not tool.parser().parse_args([]).mip
    # nine lookups of four texels of three bytes gathered and three bytes written; 12 B of indices, 36 B of vertices, 4 B written;
    # face, bary and (per face) a lod read, two lookups, 12 B written
    assert tool._mip_bytes("mip_reduce_kernel", 1000) == 1000 * (9 * 12 + 3)
    assert tool._mip_bytes("mip_lod_kernel", 1000) == 1000 * 52
    assert tool._mip_bytes("mip_sample_kernel", 1000) == 1000 * (16 + 24 + 12)


# ------------------------------------------------------------------------------------------------ levels
def test_levels_equal_the_reference_for_every_texels():
    from nerf_meets_mlx_amd.engine import mesh as E
    lib = _lib()
    out = (C.c_int32 * 7)()
    for texels in range(2, 65):
        for k in range(7):
            out[k] = -7
        assert lib.nerf_mip_levels(texels, out) == 0
        want = M.levels(texels)
        assert out[0] == len(want) <= 6 and tuple(out[1:1 + out[0]]) == want and all(x == 0 for x in out[1 + out[0]:])
        assert E.mip_levels(texels) == want and want[0] == texels and want[-1] == 2
    assert (M.levels(8), M.levels(9), M.levels(64), M.levels(2)) == ((8, 4, 2), (9, 5, 3, 2), (64, 32, 16, 8, 4, 2), (2,))
    for texels in (1, 65, 0, -1):
        assert lib.nerf_mip_levels(texels, out) == E_SHAPE and M.levels(texels) is None
        with pytest.raises(ValueError):
            E.mip_levels(texels)
    assert lib.nerf_mip_levels(8, None) == E_NULL
    for texels in (True, 8.0, "8", None):
        with pytest.raises(ValueError):
            E.mip_levels(texels)


# ------------------------------------------------------------------------------------------------ argument errors
def test_every_argument_error_returns_before_device_work():
    """Without a device the first launch would fail with NERF_E_HIP: every refusal below is NERF_E_SHAPE or NERF_E_NULL, so it was
    made before any device work.  The device pointers are never dereferenced."""
    lib = _lib()
    p = C.c_void_p(4096)
    big = (1 << 24) + 1
    good = R.view_of(R.look_at(S.CENTRE + [2.6, 1.1, 2.2], S.CENTRE), R.intrinsics(48, 64))
    nan, inf = float("nan"), float("inf")

    def red(fine=p, F=9, T_=8, coarse=p, p0=0, count=5):
        return lib.nerf_mip_reduce(fine, F, T_, coarse, p0, count, None)

    def lod(verts=p, V=10, faces=p, F=9, view=good, near=0.5, T_=8, scale=1.0, out=p):
        v = None if view is None else np.ascontiguousarray(view, np.float32).ctypes.data_as(C.POINTER(C.c_float))
        return lib.nerf_mip_lod(verts, V, faces, F, v, near, T_, scale, out, None)

    def smp(images=(4096, 4096, 4096), F=9, T_=8, face=p, bary=p, lod_=p, per_face=0, n=5, rgb=p):
        arr = None if images is None else (C.c_void_p * len(images))(*images)
        return lib.nerf_mip_sample(arr, F, T_, face, bary, lod_, per_face, n, rgb, None)

    def bad_view(q, value):
        v = good.copy()
        v[q] = value
        return v

    assert T.layout(9, 4) == (18, 12, 3, 6)
    Pn = 18 * 12                                                          # the coarse atlas of nine faces below T = 8
    shape = {"nerf_mip_reduce": [{"T_": 1}, {"T_": 2}, {"T_": 65}, {"T_": 0}, {"F": -1}, {"F": big}, {"p0": -1}, {"count": -1},
                                 {"p0": Pn - 4}, {"p0": Pn, "count": 1}, {"count": Pn + 1}, {"p0": 1 << 62, "count": 1 << 62},
                                 {"count": 30 * 20}],
             "nerf_mip_lod": [{"T_": 1}, {"T_": 65}, {"F": -1}, {"F": big}, {"V": -1}, {"V": big}, {"near": 0.0}, {"near": -1.0},
                              {"near": inf}, {"near": nan}, {"scale": 0.0}, {"scale": -1.0}, {"scale": inf}, {"scale": nan}]
             + [{"view": bad_view(q, nan)} for q in range(16)] + [{"view": bad_view(12, inf)}, {"view": bad_view(3, -inf)}],
             "nerf_mip_sample": [{"T_": 1}, {"T_": 65}, {"F": -1}, {"F": big}, {"per_face": 2}, {"per_face": -1}, {"n": -1},
                                 {"n": 1 << 31}]}
    null = {"nerf_mip_reduce": [{"fine": None}, {"coarse": None}],
            "nerf_mip_lod": [{"view": None}, {"verts": None}, {"faces": None}, {"out": None}],
            "nerf_mip_sample": [{"images": None}, {"images": (4096, 0, 4096)}, {"images": (0, 4096, 4096)}, {"images": (4096, 4096, 0)},
                                {"face": None}, {"bary": None}, {"lod_": None}, {"rgb": None}]}
    call = {"nerf_mip_reduce": red, "nerf_mip_lod": lod, "nerf_mip_sample": smp}
    for want, table in ((E_SHAPE, shape), (E_NULL, null)):
        for name, cases in table.items():
            for kw in cases:
                assert call[name](**kw) == want, (name, {k: v for k, v in kw.items() if k != "view"})
                assert name.encode() in lib.nerf_last_error(), (name, kw, lib.nerf_last_error())
    # nothing to do is no error and needs neither pointers nor a device
    assert red(count=0, fine=None, coarse=None) == 0 and red(p0=Pn, count=0) == 0
    assert lod(F=0, faces=None, out=None, verts=None, V=0) == 0
    assert smp(n=0, images=None, face=None, bary=None, lod_=None, rgb=None) == 0


def test_engine_argument_checks():
    from nerf_meets_mlx_amd.engine import mesh as E
    v, f = (torch.from_numpy(a.copy()) for a in S.sphere(12))
    mesh = E.Mesh(v, f, torch.zeros_like(v), None)
    F = f.shape[0]

    def tex(texels, **kw):
        W, H = T.layout(F, texels)[:2]
        t = E.Texture(torch.zeros(H, W, 3, dtype=torch.uint8), torch.zeros(F, 3, 2), texels)
        return t._replace(**kw)
    good = E.TexturePyramid((tex(8), tex(4), tex(2)))
    assert E._check_pyramid("t", good, mesh) == 8 and E._check_pyramid("t", E.TexturePyramid((tex(2),)), mesh) == 2
    for bad in (E.TexturePyramid((tex(8), tex(4))), E.TexturePyramid((tex(8), tex(2), tex(4))), E.TexturePyramid(()),
                E.TexturePyramid([tex(8), tex(4), tex(2)]), (tex(8), tex(4), tex(2)), tex(8), None,
                E.TexturePyramid((tex(8), tex(4), tex(2, image=torch.zeros(3, 3, 3, dtype=torch.uint8)))),
                E.TexturePyramid((tex(8), tex(4, uv=torch.zeros(F - 1, 3, 2)), tex(2))),
                E.TexturePyramid((tex(8), tex(4), tex(2), tex(2)))):
        with pytest.raises(ValueError):
            E._check_pyramid("t", bad, mesh)
    assert E.check_lod_scale(2) == 2.0 and E.check_lod_scale(np.float32(0.5)) == 0.5
    for bad in (0, -1.0, float("nan"), float("inf"), True, "1", None, 1e-50, 1e39):
        with pytest.raises(ValueError):
            E.check_lod_scale(bad)
    pose, K = R.look_at(S.CENTRE + [2.6, 1.1, 2.2], S.CENTRE), R.intrinsics(8, 8)
    for kw in ({"texels": 1}, {"texels": 65}, {"scale": 0.0}, {"near": 0.0}, {"texels": 8.5}):
        with pytest.raises(ValueError):
            E.face_lod(mesh, pose, K, **kw)
    face, bary, lod = torch.zeros(4, dtype=torch.int32), torch.zeros(4, 2), torch.zeros(4)
    for kw in ({"face": face.long()}, {"bary": bary[:3]}, {"lod": lod[:3]}, {"lod": lod.double()}, {"per_face": 1},
               {"lod": torch.zeros(F), "per_face": False}, {"lod": lod, "per_face": True}, {"pyramid": tex(8)}):
        args = {"pyramid": good, "face": face, "bary": bary, "lod": lod, "per_face": False, **kw}
        with pytest.raises(ValueError):
            E.sample_texture_mip(args["pyramid"], mesh, args["face"], args["bary"], args["lod"], args["per_face"])
    for kw in ({"lod_scale": 0.0}, {"lod_scale": float("nan")}, {"pyramid": tex(8)}, {"H": 0}):
        args = {"H": 8, "pyramid": good, **kw}
        with pytest.raises(ValueError):
            E.render_mesh_mip(mesh, pose, K, args["H"], 8, args["pyramid"], lod_scale=args.get("lod_scale", 1.0))


# ------------------------------------------------------------------------------------------------ properties of the rule
def _owners(F, texels):
    W, H = T.layout(F, texels)[:2]
    Y, X = np.mgrid[0:H, 0:W]
    return T.owner(T.layout(F, texels), X, Y)


@pytest.mark.parametrize("texels", [3, 8, 9])
def test_a_constant_atlas_stays_that_constant_at_every_level(texels):
    F = 5
    own = _owners(F, texels)[0]
    image = np.where((own < F)[..., None], np.array([77, 0, 255], np.uint8), np.uint8(0)).astype(np.uint8)
    levels = M.pyramid(image, F, texels)
    assert [tl for _, _, tl in levels] == list(M.levels(texels))
    for im, uv, tl in levels:
        used = _owners(F, tl)[0] < F
        assert (im[used] == [77, 0, 255]).all() and not im[~used].any(), tl            # the gutter included
        assert np.array_equal(uv, T.uvs(F, tl))


@pytest.mark.parametrize("texels", [3, 4, 8, 9])
@pytest.mark.parametrize("F", [1, 2, 5, 37])
def test_no_read_of_the_reduce_leaves_the_faces_texels(F, texels):
    """Every fine texel that a coarse texel reads with a weight other than 0 has the reading texel's face as its owner.  A lookup
    at a point on the hypotenuse (the corners b and c, and every point between them with integral coordinates) also loads the
    texel diagonally beyond it, with the weight 0 * 0: for the even face of a cell that is its own second gutter diagonal, for
    the odd face, which owns one gutter diagonal only, it is the even face's outermost texel.  What is multiplied by 0 does not
    reach the value; such a load stays inside the reading face's cell."""
    rng = np.random.default_rng(100 * F + texels)
    W, H = T.layout(F, texels)[:2]
    fine = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    reads = []
    M.reduce(fine, F, texels, reads)
    lf, lc = T.layout(F, texels), T.layout(F, (texels + 1) // 2)
    seen = 0
    for p, X, Y, w in reads:
        reader = T.owner(lc, p % lc[0], p // lc[0])[0]
        assert (reader < F).all()
        owner = T.owner(lf, X, Y)[0]
        assert ((owner == reader[:, None]) | (w == 0)).all()
        assert ((owner >> 1) == (reader[:, None] >> 1)).all()
        seen += int((w != 0).sum())
    assert seen > 0


@pytest.mark.parametrize("texels", [3, 8, 9])
def test_every_level_of_an_affine_field_is_within_the_bound(texels):
    """The affine colour of tests/test_gpu_texture.py baked on face-permuted sphere24: every level, looked up at 4096 random
    in-triangle samples, lies within 1.5 / 255 of the field (measured with this reference: 0.50, 0.65 and 0.50 / 255 at most for
    texels 3, 8 and 9)."""
    v, f = S.sphere(24)
    f = f[np.random.default_rng(24).permutation(len(f))]
    n = T.vertex_normals(v, f)

    def query(rows):
        raw = np.ones((len(rows), 4), F32)
        raw[:, :3] = rows[:, :3].astype(np.float64) @ AFFINE_M.T + AFFINE_C
        return raw
    image, _ = T.bake(query, v, n, f, texels)
    rng = np.random.default_rng(texels)
    sf = rng.integers(0, len(f), 4096)
    sb = rng.dirichlet([1, 1, 1], 4096)[:, 1:].astype(F32)
    for im, _, tl in M.pyramid(image, len(f), texels):
        rgb, rows = T.sample(im, v, n, f, tl, sf, sb, rows=True)
        want = rows[:, :3].astype(np.float64) @ AFFINE_M.T + AFFINE_C
        err = np.abs(rgb.astype(np.float64) - want).max()
        print("texels", texels, "level of", tl, "max |lookup - field| * 255", err * 255)
        assert err <= 1.5 / 255


def _checker_deviation(texels, H=48, W=64):
    """(through level 0, through the pyramid): the mean absolute deviation of the covered pixels from their mean, sphere24 seen at
    H x W with level 0 alternating 0 and 255 by the parity of i + j inside every face."""
    v, f = S.sphere(24)
    F = len(f)
    own, i, j = _owners(F, texels)
    image = np.where((own < F) & ((i + j) % 2 == 1), 255, 0).astype(np.uint8)[..., None].repeat(3, 2)
    images = [im for im, _, _ in M.pyramid(image, F, texels)]
    view = R.view_of(R.look_at(S.CENTRE + [2.6, 1.1, 2.2], S.CENTRE), R.intrinsics(H, W))
    rgb, face, bary, _, _, lod = M.render(v, f, view, H, W, 0.01, images, texels, np.zeros(3, F32))
    hit = face >= 0
    assert hit.sum() > 300 and np.bincount(face[hit]).max() <= 12         # a face covers a few pixels at most
    plain = T.sample(image, v, T.vertex_normals(v, f), f, texels, face, bary)
    sharp = M.sample(images, F, texels, face, bary, np.zeros(F, F32), per_face=True)
    assert np.array_equal(plain.view(np.int32), sharp.view(np.int32))     # lod 0 everywhere is the level-0 picture

    def mad(x):
        x = x[hit].astype(np.float64)
        return np.abs(x - x.mean()).mean()
    print("texels", texels, "mean absolute deviation: level 0", mad(plain), "pyramid", mad(rgb), "lod", lod[face[hit]].min(),
          lod[face[hit]].max())
    return mad(plain), mad(rgb)


def test_a_checker_aliases_less_through_the_pyramid():
    """The checker is taken at texels = 9.  The rule keeps a face's three corner texels as they are at every level (each of the
    four tap pairs of a corner has a tap outside the triangle), which keeps the levels continuous at the vertices; the coarsest
    level is those three texels.  With an odd texels the corners (0, 0), (T - 1, 0), (0, T - 1) have the same parity, so the checker
    is a constant plus a pattern at the texel frequency, which is what a minified lookup should remove: measured with this
    reference 0.125 through level 0 and 0.058 through the pyramid.  With an even texels the corners are 0, 255 and 255: the coarsest
    level is then a ramp from 0 to 255 across every face, and the deviation does not fall (texels = 8: 0.121 through level 0,
    0.130 through the pyramid; printed here, not asserted, and recorded in DESIGN.md section 34 under "Not done")."""
    _checker_deviation(8)
    plain, mip = _checker_deviation(9)
    assert mip < plain
