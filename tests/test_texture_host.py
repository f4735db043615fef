"""The texture atlas without a GPU: the layout rule of include/nerf_hip.h "texture atlas" (nerf_texture_layout is a host call)
against tests/_texture_ref.py, the ownership and bilinear-footprint properties of the rule in numpy, the argument checks of the C
ABI (they return before any device work, so they run here) and of engine.mesh, the OBJ / MTL / PNG writer and reader, and the
header / binding / pipeline bookkeeping.  The kernels are held to the reference bit for bit in tests/test_gpu_texture.py."""
import ctypes as C
import inspect
import os
import re
import struct
import zlib

import numpy as np
import pytest
import torch

from tests import _smooth_ref as S
from tests import _texture_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE = -1, -2
ENTRIES = ["nerf_texture_layout", "nerf_texture_rows", "nerf_texture_sample", "nerf_texture_store", "nerf_texture_uv"]


def _lib():
    from nerf_meets_mlx_amd import _native
    return _native.lib()


# ------------------------------------------------------------------------------------------------ bookkeeping
def test_header_section_bindings_and_makefile():
    from nerf_meets_mlx_amd import _native
    text = open(os.path.join(ROOT, "include", "nerf_hip.h")).read()
    start = text.index("/* ---------------------------------------------------------------- texture atlas (no reference counterpart)")
    assert text.index("mesh smoothing (no reference counterpart)") < start < text.index("fused renderer (a14 / a18)")
    section = text[start:text.index("/* ----", start + 1)]
    decl = re.sub(r"/\*.*?\*/", "", section, flags=re.S)
    assert sorted(set(re.findall(r"\b(nerf_texture_[a-z_]+)\s*\(", decl))) == ENTRIES
    assert "#define NERF_TEXTURE_MAX_SIDE 16384" in decl and "#define NERF_ABI_VERSION 3" in text
    lib = _lib()
    for e in ENTRIES:
        assert e in _native.SIGNATURES and hasattr(lib, e)
    for word in ("i + j <= S - 1", "wa = (1 - wb) - wc", "((w00 c00 + w10 c10) + w01 c01) + w11 c11", "Not done", "mipmaps"):
        assert word in section, word
    mk = open(os.path.join(ROOT, "nerf_meets_mlx_amd", "csrc", "Makefile")).read()
    srcs = next(ln for ln in mk.splitlines() if ln.startswith("SRCS"))
    assert "texture.hip" in srcs.split() and "texture.h" in next(ln for ln in mk.splitlines() if ln.startswith("HDRS")).split()
    src = open(os.path.join(ROOT, "nerf_meets_mlx_amd", "csrc", "texture.hip")).read()
    kernels = sorted(set(re.findall(r"\b(\w+_kernel)\(", src)))
    assert kernels == ["tex_rows_kernel", "tex_sample_kernel", "tex_store_kernel", "tex_uv_kernel"]
    assert "atomic" not in re.sub(r"//.*", "", src)


def test_pipeline_signatures_and_mesh_fields_are_what_they_were():
    from nerf_meets_mlx_amd.engine import mesh as E
    from nerf_meets_mlx_amd.engine.ngp import NGPTrainer
    from nerf_meets_mlx_amd.engine.trainer import Trainer
    want = [("simplify_grid", 0), ("simplify_placement", "quadric"), ("smooth_iterations", 0), ("smooth_lambda", 0.5), ("smooth_mu", -0.53)]
    for fn in (E.extract, E.mesh_volume, Trainer.extract_mesh, NGPTrainer.extract_mesh_tsdf):
        p = list(inspect.signature(fn).parameters.values())
        assert [(q.name, q.default) for q in p[-5:]] == want, fn.__qualname__
        assert not any("tex" in q.name for q in p)
    assert E.Mesh._fields == ("verts", "faces", "normals", "colors") and E.Texture._fields == ("image", "uv", "texels")
    p = inspect.signature(E.bake_texture).parameters
    assert list(p) == ["query", "mesh", "texels", "chunk", "mark"] and (p["texels"].default, p["chunk"].default) == (8, E.CHUNK)
    assert list(inspect.signature(E.sample_texture).parameters) == ["texture", "mesh", "face", "bary", "rows"]
    p = inspect.signature(Trainer.texture_mesh).parameters
    assert list(p) == ["self", "mesh", "texels"] and p["texels"].default == 8
    assert NGPTrainer.texture_mesh is Trainer.texture_mesh


def test_mesh_tool_knows_the_texture_kernels_and_flag(tmp_path, capsys):
    import argparse
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("ngp_mesh_tool", os.path.join(ROOT, "tools", "ngp_mesh.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    kernels = ["tex_rows_kernel", "tex_sample_kernel", "tex_store_kernel", "tex_uv_kernel"]
    path = tmp_path / "trace.csv"
    with open(path, "w") as fh:
        fh.write('"Kernel_Name","Start_Timestamp","End_Timestamp","Grid_Size_X"\n')
        for i, k in enumerate(kernels):
            for rep in range(2):
                fh.write(f'"void nerf::(anonymous namespace)::{k}(float const*, int)",{1000 * i},{1000 * i + 500 + 1000 * rep},{256 * (i + 1)}\n')
    tool.stats(argparse.Namespace(stats=str(path), from_=None, out=None))
    recs = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert sorted(r["kernel"] for r in recs) == kernels and all(r["launches"] == 2 and r["avg_us"] == 1.0 for r in recs)
    assert tool.parser().parse_args(["--texture", "4", "--texture", "8"]).texture == [4, 8]
    assert tool.parser().parse_args([]).texture is None
    assert tool._texture_bytes("tex_rows_kernel", 1000) == 44 * 1000 and tool._texture_bytes("tex_store_kernel", 1000) == 19 * 1000


# ------------------------------------------------------------------------------------------------ the layout
@pytest.mark.parametrize("F", [0, 1, 2, 3, 8, 9, 1000, 1 << 24])
@pytest.mark.parametrize("texels", [2, 3, 8, 64])
def test_layout_equals_the_reference_or_refuses(F, texels):
    from nerf_meets_mlx_amd.engine import mesh as E
    lib = _lib()
    out = (C.c_int64 * 4)()
    want = T.layout(F, texels)
    rc = lib.nerf_texture_layout(F, texels, out)
    if want is None:
        cells = (F + 1) // 2
        Cn = next(c for c in range(1, 4000) if c * c >= cells)
        assert Cn * (texels + 2) > 16384
        assert rc == E_SHAPE
        msg = lib.nerf_last_error().decode()
        assert "nerf_texture_layout" in msg and f"largest texels that fits is {16384 // Cn - 2}" in msg
        with pytest.raises(ValueError, match="largest texels that fits"):
            E.texture_layout(F, texels)
        return
    assert rc == 0 and tuple(out) == want == E.texture_layout(F, texels)
    W, H, Cn, Sn = want
    cells = (F + 1) // 2
    assert Sn == texels + 2 and Cn >= 1 and Cn * Cn >= cells and (Cn == 1 or (Cn - 1) ** 2 < cells)
    assert W == Cn * Sn and H == max(1, -(-cells // Cn)) * Sn and (H // Sn) * Cn >= cells > (H // Sn - 1) * Cn - (cells == 0)


def test_the_refusals_are_the_expected_ones():
    """At 2^24 faces 2897 cells a row leave 5 texels a cell: T = 2 and 3 fit, 8 and 64 do not; 1000 faces fit at every T."""
    assert [T.layout(1 << 24, t) is None for t in (2, 3, 8, 64)] == [False, False, True, True]
    assert all(T.layout(F, t) is not None for F in (0, 1, 2, 3, 8, 9, 1000) for t in (2, 3, 8, 64))
    assert T.layout(0, 8) == (10, 10, 1, 10) and T.layout(5, 2) == (8, 8, 2, 4)


@pytest.mark.parametrize("texels", [2, 3, 8])
@pytest.mark.parametrize("F", [1, 2, 5, 37])
def test_ownership_partitions_every_cell_and_no_footprint_leaves_its_face(F, texels):
    lay = T.layout(F, texels)
    W, H, Cn, Sn = lay
    Y, X = np.mgrid[0:H, 0:W]
    f, i, j = T.owner(lay, X.ravel(), Y.ravel())
    # every cell: S (S + 1) / 2 texels of the even face, S (S - 1) / 2 of the odd one, and place() is owner()'s inverse
    counts = np.bincount(f, minlength=2 * Cn * (H // Sn))
    assert (counts[0::2] == Sn * (Sn + 1) // 2).all() and (counts[1::2] == Sn * (Sn - 1) // 2).all()
    bx, by = T.place(lay, f, i, j)
    assert np.array_equal(bx, X.ravel()) and np.array_equal(by, Y.ravel())
    assert (i + j <= Sn - 1 - (f & 1)).all() and i.min() == 0 and j.min() == 0
    # dense barycentric samples of every face, edges and corners included: the texels with a non-zero weight are the face's own
    k = 4 * (texels - 1) + 3
    a, b = np.meshgrid(np.arange(k + 1), np.arange(k + 1))
    keep = a + b <= k
    bary = np.stack([a[keep] / k, b[keep] / k], 1).astype(np.float32)
    bary = np.concatenate([bary, np.random.default_rng(texels).dirichlet([1, 1, 1], 200)[:, 1:].astype(np.float32)])
    for face in range(F):
        wb, wc = T.clamp_bary(bary)
        fx, fy, w = T.footprint(lay, texels, np.full(len(wb), face), wb, wc)
        assert fx.min() >= 0 and fx.max() < W and fy.min() >= 0 and fy.max() < H
        own = T.owner(lay, fx, fy)[0]
        assert ((own == face) | (w == 0)).all(), face
        assert np.abs(w.sum(1) - 1).max() < 1e-6 and w.min() >= 0


@pytest.mark.parametrize("texels", [2, 3, 8])
def test_reference_lookup_of_an_affine_field_stays_within_the_quantisation(texels):
    """The property the GPU test rests on, on the reference alone: gutters are extrapolated, so a bilinear lookup reproduces an
    affine colour up to half a byte step of a convex combination (0.5 / 255) and float32 rounding (1e-5)."""
    v, f = S.sphere(12)
    f = f[np.random.default_rng(5).permutation(len(f))]
    nrm = T.vertex_normals(v, f)
    M, c0 = np.array([[0.1, 0.05, -0.08], [-0.06, 0.1, 0.07], [0.04, -0.09, 0.1]]), np.array([0.5, 0.42, 0.3])
    field = lambda x: x.astype(np.float64) @ M.T + c0
    image, _ = T.bake(lambda rows: np.concatenate([field(rows[:, :3]), np.ones((len(rows), 1))], 1).astype(np.float32), v, nrm, f, texels)
    rng = np.random.default_rng(6)
    bary = np.concatenate([[[0, 0], [1, 0], [0, 1], [0.5, 0], [0, 0.5], [0.5, 0.5]], rng.dirichlet([1, 1, 1], 20)[:, 1:]]).astype(np.float32)
    sf = np.repeat(np.arange(len(f)), len(bary))
    sb = np.tile(bary, (len(f), 1))
    rgb, rows = T.sample(image, v, nrm, f, texels, sf, sb, rows=True)
    want = field(rows[:, :3])
    assert 0.1 <= want.min() and want.max() <= 0.9
    assert np.abs(rgb - want).max() <= 0.5 / 255 + 1e-5


# ------------------------------------------------------------------------------------------------ argument errors
def test_every_argument_error_returns_before_device_work():
    """Without a device the first launch would fail with NERF_E_HIP: every refusal below is NERF_E_SHAPE or NERF_E_NULL, so it was
    made before any device work.  The pointers are never dereferenced."""
    lib = _lib()
    p = C.c_void_p(4096)
    big = (1 << 24) + 1
    out = (C.c_int64 * 4)()

    def rows(verts=p, normals=p, V=10, faces=p, F=9, T_=8, p0=0, count=5, out_=p):
        return lib.nerf_texture_rows(verts, normals, V, faces, F, T_, p0, count, out_, None)

    def store(raw=p, V=10, faces=p, F=9, T_=8, p0=0, count=5, image=p):
        return lib.nerf_texture_store(raw, V, faces, F, T_, p0, count, image, None)

    def uv(F=9, T_=8, out_=p):
        return lib.nerf_texture_uv(F, T_, out_, None)

    def sample(image=p, verts=p, normals=p, V=10, faces=p, F=9, T_=8, sf=p, bary=p, n=5, rgb=p, rows_=p):
        return lib.nerf_texture_sample(image, verts, normals, V, faces, F, T_, sf, bary, n, rgb, rows_, None)

    assert T.layout(9, 8) == (30, 20, 3, 10)                            # 9 faces: 5 cells, 3 a row, 2 rows
    P = 30 * 20
    shape = {"nerf_texture_layout": [lambda: lib.nerf_texture_layout(-1, 8, out), lambda: lib.nerf_texture_layout(big, 8, out),
                                     lambda: lib.nerf_texture_layout(9, 1, out), lambda: lib.nerf_texture_layout(9, 65, out),
                                     lambda: lib.nerf_texture_layout(1 << 24, 8, out)],
             "nerf_texture_rows": [lambda kw=kw: rows(**kw) for kw in ({"V": -1}, {"V": big}, {"F": -1}, {"F": big}, {"T_": 1}, {"T_": 65},
                                                                     {"p0": -1}, {"count": -1}, {"p0": P, "count": 1}, {"count": P + 1},
                                                                     {"p0": 1 << 62, "count": 1 << 62}, {"F": 1 << 24})],
             "nerf_texture_store": [lambda kw=kw: store(**kw) for kw in ({"V": -1}, {"F": big}, {"T_": 0}, {"p0": -1}, {"count": -1},
                                                                       {"p0": P - 4, "count": 5}, {"raw": C.c_void_p(4100)})],
             "nerf_texture_uv": [lambda kw=kw: uv(**kw) for kw in ({"F": -1}, {"F": big}, {"T_": 1}, {"T_": 100}, {"F": 1 << 24})],
             "nerf_texture_sample": [lambda kw=kw: sample(**kw) for kw in ({"V": big}, {"F": -1}, {"T_": 1}, {"n": -1}, {"n": 1 << 31})]}
    for name, calls in shape.items():
        for k, call in enumerate(calls):
            assert call() == E_SHAPE, (name, k)
            assert name.encode() in lib.nerf_last_error(), (name, k, lib.nerf_last_error())
    null = {"nerf_texture_layout": [lambda: lib.nerf_texture_layout(9, 8, None)],
            "nerf_texture_rows": [lambda kw=kw: rows(**kw) for kw in ({"verts": None}, {"normals": None}, {"faces": None}, {"out_": None})],
            "nerf_texture_store": [lambda kw=kw: store(**kw) for kw in ({"raw": None}, {"faces": None}, {"image": None})],
            "nerf_texture_uv": [lambda: uv(out_=None)],
            "nerf_texture_sample": [lambda kw=kw: sample(**kw) for kw in ({"image": None}, {"sf": None}, {"bary": None}, {"rgb": None},
                                                                        {"verts": None}, {"normals": None}, {"faces": None})]}
    for name, calls in null.items():
        for k, call in enumerate(calls):
            assert call() == E_NULL, (name, k)
            assert name.encode() in lib.nerf_last_error(), (name, k)
    # nothing to do is no error, and needs neither pointers nor a device
    assert rows(count=0, out_=None) == 0 and store(count=0, raw=None, image=None) == 0 and uv(F=0, out_=None) == 0
    assert sample(n=0, image=None, rgb=None) == 0 and rows(p0=P, count=0) == 0
    assert store(count=0, raw=C.c_void_p(4100)) == 0                    # (nothing is read: the alignment does not matter)


def test_engine_argument_checks():
    from nerf_meets_mlx_amd.engine import mesh as E
    v, f = (torch.from_numpy(a.copy()) for a in S.sphere(12))
    n = torch.zeros_like(v)
    good = E.Mesh(v, f, n, None)
    assert E.check_texture_args(good, 8) == (8, T.layout(len(f), 8))
    assert E.check_texture_args(good._replace(colors=n), np.int64(2))[0] == 2 and E.check_texture_args(good, 64)[0] == 64
    for t in (1, 0, -3, 65, 8.0, True, None, "8"):
        with pytest.raises(ValueError, match="texels"):
            E.check_texture_args(good, t)
    bad = [good._replace(verts=v.double()), good._replace(faces=f.long()), good._replace(normals=n[:-1]),
           good._replace(colors=n[:, :2]), good._replace(verts=v.t().contiguous().t()), good._replace(faces=f[:, :2]),
           good._replace(normals=None), good._replace(verts=v.numpy()), (v, f)]
    for m in bad:
        with pytest.raises(ValueError):
            E.check_texture_args(m, 8)
        with pytest.raises(ValueError):
            E.bake_texture(lambda r, z: None, m, 8)
    many = E.Mesh(v, torch.zeros(200001, 3, dtype=torch.int32), n)      # 100001 cells -> C = 317; 317 * 66 > 16384
    with pytest.raises(ValueError, match="largest texels that fits is 49"):
        E.check_texture_args(many, 64)
    assert E.check_texture_args(many, 49)[1][0] == 317 * 51
    tex = E.Texture(torch.zeros(T.layout(len(f), 2)[1], T.layout(len(f), 2)[0], 3, dtype=torch.uint8), torch.zeros(len(f), 3, 2), 2)
    for broken in (tex._replace(image=tex.image[:-1]), tex._replace(uv=tex.uv[:-1]), tex._replace(texels=3), tex._replace(image=tex.image.float()),
                   (tex.image, tex.uv, 2)):
        with pytest.raises(ValueError):
            E.write_obj("/nonexistent/x.obj", good, broken)
        with pytest.raises(ValueError):
            E.sample_texture(broken, good, torch.zeros(1, dtype=torch.int32), torch.zeros(1, 2))
    for face, bary in ((torch.zeros(2, dtype=torch.int64), torch.zeros(2, 2)), (torch.zeros(2, dtype=torch.int32), torch.zeros(2, 3)),
                       (torch.zeros(2, dtype=torch.int32), torch.zeros(3, 2)), (torch.zeros(2, 1, dtype=torch.int32), torch.zeros(2, 2))):
        with pytest.raises(ValueError):
            E.sample_texture(tex, good, face, bary)


def test_no_faces_gives_a_black_cell_and_no_query():
    from nerf_meets_mlx_amd.engine import mesh as E
    v = torch.from_numpy(S.tetrahedron()[0].copy())
    m = E.Mesh(v, torch.zeros(0, 3, dtype=torch.int32), torch.zeros_like(v))

    def query(rows, z):
        raise AssertionError("queried")
    tex = E.bake_texture(query, m, 6)
    assert tex.image.shape == (8, 8, 3) and tex.image.dtype == torch.uint8 and not tex.image.any()
    assert tex.uv.shape == (0, 3, 2) and tex.texels == 6


# ------------------------------------------------------------------------------------------------ OBJ, MTL, PNG
def _decode_png_with_zlib_alone(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + body)
        chunks.append((kind, body))
        pos += 12 + n
    assert [k for k, _ in chunks][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    W, H, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    lines = np.frombuffer(zlib.decompress(b"".join(b for k, b in chunks if k == b"IDAT")), np.uint8).reshape(H, 1 + 3 * W)
    assert not lines[:, 0].any()                                        # filter type 0 on every row
    return lines[:, 1:].reshape(H, W, 3)


@pytest.mark.parametrize("name,texels", [("tetrahedron", 2), ("sphere12", 3), ("soup", 8)])
def test_obj_round_trip_byte_for_byte(tmp_path, name, texels):
    from nerf_meets_mlx_amd.engine import mesh as E
    rng = np.random.default_rng(9)
    if name == "soup":
        v, f = rng.standard_normal((40, 3)).astype(np.float32) * 1e3, rng.integers(0, 40, (37, 3)).astype(np.int32)
        v[0] = [np.float32(1e-30), np.float32(-3.4e38), np.float32(1) + np.finfo(np.float32).eps]
    else:
        v, f = S.tetrahedron() if name == "tetrahedron" else S.sphere(12)
    nrm = T.vertex_normals(v, f)
    W, H = T.layout(len(f), texels)[:2]
    image = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    mesh = E.Mesh(torch.from_numpy(v.copy()), torch.from_numpy(f.copy()), torch.from_numpy(nrm), torch.rand(len(v), 3))
    tex = E.Texture(torch.from_numpy(image), torch.from_numpy(T.uvs(len(f), texels)), texels)
    path = str(tmp_path / f"{name}.obj")
    assert E.write_obj(path, mesh, tex) == path
    assert sorted(os.listdir(tmp_path)) == [f"{name}.mtl", f"{name}.obj", f"{name}.png"]          # no temporary file is left
    back, btex = E.read_obj(path)
    for a, b in ((back.verts, mesh.verts), (back.normals, mesh.normals), (btex.uv, tex.uv)):
        assert a.dtype == b.dtype and a.shape == b.shape and a.numpy().tobytes() == b.numpy().tobytes()
    assert back.faces.dtype == torch.int32 and torch.equal(back.faces, mesh.faces) and back.colors is None
    assert btex.image.dtype == torch.uint8 and torch.equal(btex.image, tex.image) and btex.texels == texels
    assert np.array_equal(_decode_png_with_zlib_alone(open(tmp_path / f"{name}.png", "rb").read()), image)
    lines = open(path).read().splitlines()
    kinds = [ln.split()[0] for ln in lines]
    assert kinds.count("v") == len(v) == kinds.count("vn") and kinds.count("vt") == 3 * len(f) and kinds.count("f") == len(f)
    k = len(f) - 1
    a, b, c = (int(x) + 1 for x in f[k])
    assert lines[-1] == f"f {a}/{3 * k + 1}/{a} {b}/{3 * k + 2}/{b} {c}/{3 * k + 3}/{c}"
    assert f"mtllib {name}.mtl" in lines and "usemtl atlas" in lines
    mtl = open(tmp_path / f"{name}.mtl").read().splitlines()
    assert mtl[0] == "newmtl atlas" and f"map_Kd {name}.png" in mtl and sum(ln.startswith("newmtl") for ln in mtl) == 1
    src = inspect.getsource(E)
    assert not re.search(r"^\s*(import|from)\s+(PIL|imageio|cv2|matplotlib|skimage)", src, flags=re.M)
