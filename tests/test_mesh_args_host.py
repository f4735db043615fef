"""The argument surface of the mesh layer (nerf_meets_mlx_amd/engine/mesh) on the host, against a recording of itself from before
its checks were folded onto one vocabulary: every `check_*` function, `tsdf_views`, `texture_layout`,
`mip_levels` and every public function that takes tensors, called with CPU tensors.  Per integer parameter a bool, an integral
float, a numpy integer, lo - 1, lo, hi, hi + 1, a string and None; per real parameter a bool, NaN, +-inf, 0, -0.0, a string, a
numpy float32, a double beyond float32 and, where the check rounds to float32, one that rounds to 0; per tensor parameter not a
tensor, another dtype, another rank, another trailing shape, another row count, not contiguous and another device (`meta`); per
pair of adjacent checks one call that fails both, which pins their order.  A call that passes every check and would launch ends in
`_native.ptr`'s ValueError ("no CPU path"): that it is this error and no other records that the checks passed; a call with
nothing to do (V = 0, F = 0, n = 0, one mip level) returns, and its result is recorded as dtypes and shapes.
`python -m tests.test_mesh_args_host` at the parent commit wrote tests/golden/mesh_args_parent.json (every distinct outcome once,
the calls as indices); the test makes the same calls on the code under test.  Needs the built library (`texture_layout`,
`mip_levels` and the workspace sizes are host entries of it), no GPU.

Two calls are left out on purpose: `Trainer.extract_mesh` with a bad `simplify_placement` AND a bad smoothing argument (the
placement is refused first since section 36, the smoothing argument was before), and `extract` with an unhashable
`simplify_placement` (a TypeError of the dict lookup before, the placement's ValueError since)."""
import json
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

from nerf_meets_mlx_amd.engine import mesh as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mesh_args_parent.json")
NO_CPU_PATH = "ValueError: libnerf_hip kernels need tensors on the ROCm device (there is no CPU path)"
LO, HI = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]
BIG = (1 << 24) + 1


# ------------------------------------------------------------------------------------------------ values
def vals(*xs):
    return [(repr(x), x) for x in xs]


def ints(lo, hi):
    """The cases of an integer parameter that is accepted in [lo, hi]."""
    return vals(True, float(lo), np.int32(lo), np.int64(hi), lo - 1, lo, hi, hi + 1, "3", None)


def reals(*more, tiny=False):
    """The cases of a real parameter; `tiny`: also a double that rounds to 0 as a float32."""
    return vals(True, math.nan, math.inf, -math.inf, 0, -0.0, "1", np.float32(0.5), np.float64(0.25), 1e39, None, *more, *([1e-50] if tiny else []))


def bools():
    return vals(1, 0, None, "yes", np.bool_(True))


def other_dtype(t):
    return {torch.float32: torch.float64, torch.int32: torch.int64, torch.int64: torch.int32, torch.uint8: torch.int32}[t.dtype]


def tfaults(t):
    """The faults of a tensor parameter whose valid value is `t` (more than one element)."""
    out = [("a list", t.tolist()), ("dtype", t.to(other_dtype(t))), ("rank", t.reshape(-1) if t.dim() > 1 else t[None]),
           ("rows", torch.cat([t, t[:1]])), ("strided", torch.stack([t, t], -1)[..., 0]), ("meta", t.to("meta"))]
    if t.dim() > 1:
        out.append(("wider", torch.cat([t, t.narrow(-1, 0, 1)], -1)))
    assert not out[4][1].is_contiguous() and out[4][1].shape == t.shape
    return out


BOXES = [("len 2", [0.0, 0.0]), ("len 2 nan", [math.nan, 0.0]), ("nan", [math.nan, -1.0, -1.0]), ("inf", [-math.inf, -1.0, -1.0]),
         ("lo = hi", [1.0, -1.0, -1.0]), ("a string", ["a", 0.0, 0.0]), ("None", None), ("ints", [-2, -2, -2])]


def make_mesh(V=4, F=2, colors=True):
    verts = torch.arange(3 * V, dtype=torch.float32).reshape(V, 3) / 16
    faces = (torch.arange(3 * F, dtype=torch.int32).reshape(F, 3) % max(V, 1))
    return E.Mesh(verts, faces, verts.clone(), verts.clone() if colors else None)


def make_texture(F, T, value=7):
    W, H, _, _ = E.texture_layout(F, T)
    return E.Texture(torch.full((H, W, 3), value, dtype=torch.uint8), torch.zeros(F, 3, 2, dtype=torch.float32), T)


def make_pyramid(F, T):
    return E.TexturePyramid(tuple(make_texture(F, t) for t in E.mip_levels(T)))


def mesh_faults(mesh):
    """[(tag, Mesh)]: every tensor fault of every field, in the order _check_mesh_tensors looks at them."""
    out = [("not a Mesh", tuple(mesh))]
    for field in ("verts", "faces", "normals", "colors"):
        out += [(f"{field} {tag}", mesh._replace(**{field: bad})) for tag, bad in tfaults(getattr(mesh, field))]
    out.append(("no colors", mesh._replace(colors=None)))
    for a, b in (("verts", "faces"), ("faces", "normals"), ("normals", "colors")):
        out.append((f"{a} + {b} dtype", mesh._replace(**{a: getattr(mesh, a).to(other_dtype(getattr(mesh, a))),
                                                       b: getattr(mesh, b).to(other_dtype(getattr(mesh, b)))})))
    return out


def texture_faults(tex):
    out = [("not a Texture", tuple(tex)), ("texels 1", tex._replace(texels=1)), ("texels True", tex._replace(texels=True)),
           ("texels 65", tex._replace(texels=65)), ("other texels", tex._replace(texels=tex.texels + 1))]
    for field in ("image", "uv"):
        out += [(f"{field} {tag}", tex._replace(**{field: bad})) for tag, bad in tfaults(getattr(tex, field))]
    out.append(("texels 1 + image dtype", tex._replace(texels=1, image=tex.image.to(torch.int32))))
    out.append(("image + uv dtype", tex._replace(image=tex.image.to(torch.int32), uv=tex.uv.to(torch.float64))))
    return out


def pyramid_faults(pyr):
    out = [("not a pyramid", tuple(pyr)), ("a list of levels", E.TexturePyramid(list(pyr.levels))), ("no levels", E.TexturePyramid(())),
           ("level 0 alone", E.TexturePyramid(pyr.levels[:1])), ("levels swapped", E.TexturePyramid(pyr.levels[::-1]))]
    for k, level in enumerate(pyr.levels):
        for tag, bad in texture_faults(level)[:3] + texture_faults(level)[5:7]:
            out.append((f"level {k} {tag}", E.TexturePyramid(pyr.levels[:k] + (bad,) + pyr.levels[k + 1:])))
    return out


# ------------------------------------------------------------------------------------------------ the table
def sweep(rows, name, fn, base, cases, order=(), bad=None):
    """fn(**base) as it is; with each parameter of `cases` replaced by each of its (tag, value); and for every adjacent pair of
    `order` with both replaced by their `bad` value."""
    rows.append((f"{name}: valid", fn, dict(base)))
    for p, cs in cases.items():
        for tag, v in cs:
            rows.append((f"{name}: {p} = {tag}", fn, dict(base, **{p: v})))
    for p, q in zip(order, order[1:]):
        rows.append((f"{name}: bad {p} + bad {q}", fn, dict(base, **{p: bad[p], q: bad[q]})))


def _tsdf_init(**kw):
    return E.TSDFVolume(**kw)


def _fake_trainer():
    return types.SimpleNamespace(_mesh_box=lambda aabb: (LO, HI), _mesh_field=lambda: (None, E.RELU), device="cpu", far=6.0, H=4, W=4,
                                 K=np.array([[5.0, 0, 2], [0, 5.0, 2], [0, 0, 1]]), poses=np.eye(4)[None], render_depth=None)


def _trainer_extract(**kw):
    from nerf_meets_mlx_amd.engine.trainer import Trainer
    return Trainer.extract_mesh(_fake_trainer(), **kw)


def _trainer_extract_tsdf(**kw):
    from nerf_meets_mlx_amd.engine.ngp import NGPTrainer
    return NGPTrainer.extract_mesh_tsdf(_fake_trainer(), **kw)


def table():
    """[(label, function, keyword arguments)]"""
    rows = []
    mesh, mesh0, bare = make_mesh(), make_mesh(0, 0), make_mesh(colors=False)
    F, T = mesh.faces.shape[0], 4
    tex, tex0, tex2 = make_texture(F, T), make_texture(0, T), make_texture(F, 2)
    pyr, pyr0 = make_pyramid(F, T), make_pyramid(0, T)
    vol = torch.zeros(4, 4, 4, dtype=torch.float32)
    c2w = np.concatenate([np.eye(3), [[0.0], [0.0], [3.0]]], 1)
    K = np.array([[5.0, 0, 2], [0, 5.0, 2], [0, 0, 1]])
    bad_box = [0.0, 0.0]
    mf, tf, pf = mesh_faults(mesh), texture_faults(tex), pyramid_faults(pyr)
    bad_mesh, bad_tex, bad_pyr = mf[2][1], tf[1][1], pf[0][1]

    # -- the volume stage
    sweep(rows, "check_mesh_args", E.check_mesh_args, dict(resolution=4, lo=LO, hi=HI, iso=0.5),
          dict(resolution=ints(2, E.MAX_RES), lo=BOXES, hi=BOXES[:3] + BOXES[5:7], iso=reals(2, -3.5)),
          ["resolution", "lo", "iso"], dict(resolution=1, lo=bad_box, iso=math.nan))
    rows.append(("check_mesh_args: iso default", E.check_mesh_args, dict(resolution=np.int64(7), lo=(0, 0, 0), hi=(1, 2, 3))))
    sweep(rows, "check_component_args", E.check_component_args, dict(min_component=3, largest_only=False, resolution=4),
          dict(min_component=ints(0, 64), largest_only=bools()), ["min_component", "largest_only"], dict(min_component=-1, largest_only=1))
    sweep(rows, "check_opening_args", E.check_opening_args, dict(opening_radius=2), dict(opening_radius=ints(0, E.MAX_OPENING_RADIUS)))
    rows.append(("density_volume: activation 2", E.density_volume, dict(query=None, activation=2, resolution=4, lo=LO, hi=HI, device="cpu")))
    rows.append(("density_volume: resolution 1 + activation 2", E.density_volume, dict(query=None, activation=2, resolution=1, lo=LO, hi=HI, device="cpu")))
    rows.append(("density_volume: valid", E.density_volume, dict(query=None, activation=E.EXP, resolution=4, lo=LO, hi=HI, device="cpu")))
    volumes = tfaults(vol)[:3] + tfaults(vol)[4:6] + [("not a cube", torch.zeros(4, 4, 5)), ("R = 1", torch.zeros(1, 1, 1)), ("R = 2", torch.zeros(2, 2, 2))]
    bad_vol = torch.zeros(4, 4)
    sweep(rows, "marching_cubes", E.marching_cubes, dict(volume=vol, iso=0.5, lo=LO, hi=HI),
          dict(volume=volumes, iso=reals(), lo=BOXES), ["volume", "lo", "iso"], dict(volume=bad_vol, lo=bad_box, iso=math.nan))
    sweep(rows, "connected_components", E.connected_components, dict(volume=vol, iso=0.5), dict(volume=volumes, iso=reals()),
          ["volume", "iso"], dict(volume=bad_vol, iso=math.nan))
    comps = E.Components(torch.zeros(4, 4, 4, dtype=torch.int32), torch.zeros(4, 4, 4, dtype=torch.int32), torch.zeros(3, dtype=torch.int64))
    comp_cases = [("a tuple", tuple(comps))]
    for field in comps._fields:
        comp_cases += [(f"{field} {tag}", comps._replace(**{field: b})) for tag, b in tfaults(getattr(comps, field))]
    sweep(rows, "filter_components", E.filter_components, dict(volume=vol, iso=0.5, min_component=2, largest_only=False, components=comps),
          dict(volume=volumes, iso=reals(), min_component=ints(0, 64), largest_only=bools(), components=comp_cases + [("None", None)]),
          ["volume", "iso", "min_component", "largest_only", "components"],
          dict(volume=bad_vol, iso=math.nan, min_component=-1, largest_only=1, components=comp_cases[2][1]))
    sweep(rows, "erode", E.erode, dict(volume=vol, iso=0.5, radius=1), dict(volume=volumes, iso=reals(), radius=ints(1, E.MAX_OPENING_RADIUS)),
          ["volume", "iso", "radius"], dict(volume=bad_vol, iso=math.nan, radius=0))
    sweep(rows, "reconstruct", E.reconstruct, dict(volume=vol, kept=vol.clone(), iso=0.5, radius=1),
          dict(volume=volumes, kept=tfaults(vol), iso=reals(), radius=ints(1, E.MAX_OPENING_RADIUS)),
          ["volume", "iso", "radius", "kept"], dict(volume=bad_vol, iso=math.nan, radius=0, kept=bad_vol))
    sweep(rows, "open_components", E.open_components, dict(volume=vol, iso=0.5, radius=1, min_component=2, largest_only=True),
          dict(volume=volumes, iso=reals(), radius=ints(1, E.MAX_OPENING_RADIUS), min_component=ints(0, 64), largest_only=bools()),
          ["volume", "iso", "radius", "min_component", "largest_only"], dict(volume=bad_vol, iso=math.nan, radius=0, min_component=-1, largest_only=1))

    # -- TSDF
    tsdf_order = ["trunc", "acc_min", "far", "carve", "min_views", "H", "W"]
    tsdf_bad = dict(trunc=0.0, acc_min=0.0, far=0.0, carve=1, min_views=0, H=0, W=0)
    sweep(rows, "check_tsdf_args", E.check_tsdf_args, dict(trunc=0.1, acc_min=0.5, far=6.0, carve=True, min_views=2, H=48, W=64),
          dict(trunc=reals(-1.0, 0.5), acc_min=reals(1.0, 1.5, -0.5), far=reals(-1.0, 2), carve=bools(), min_views=ints(1, 1 << 40),
               H=ints(1, 1 << 24), W=ints(1, 1 << 24)), tsdf_order, tsdf_bad)
    rows.append(("check_tsdf_args: defaults", E.check_tsdf_args, {}))
    stack = np.stack([c2w, c2w])
    full = np.concatenate([c2w, [[0, 0, 0, 1.0]]])
    c2ws = [("[3, 4]", c2w), ("[4, 4]", full), ("[2, 3, 4]", stack), ("[2, 4, 4]", np.stack([full, full])), ("a tensor", torch.tensor(c2w)),
            ("a float32 tensor stack", torch.tensor(stack, dtype=torch.float32)), ("lists", c2w.tolist()), ("[0, 3, 4]", stack[:0]),
            ("[5, 4]", np.zeros((5, 4))), ("[3, 3]", np.eye(3)), ("[12]", c2w.reshape(-1)), ("[1, 2, 3, 4]", stack[None]), ("nan", c2w * math.nan),
            ("inf", c2w * 1e39), ("None", None), ("a string", "pose")]
    Ks = [("a tensor", torch.tensor(K)), ("lists", K.tolist()), ("[2, 2]", np.eye(2)), ("[1, 3, 3]", K[None]), ("nan", K * math.nan),
          ("beyond float32", K * 1e39), ("inexact in float32", K / 3), ("None", None)]
    sweep(rows, "tsdf_views", E.tsdf_views, dict(c2w=c2w, K=K), dict(c2w=c2ws, K=Ks), ["c2w", "K"], dict(c2w=np.eye(3), K=np.eye(2)))
    rows.append(("tsdf_views: nan c2w + bad K", E.tsdf_views, dict(c2w=c2w * math.nan, K=np.eye(2))))
    sweep(rows, "TSDFVolume", _tsdf_init, dict(resolution=4, lo=LO, hi=HI, trunc=0.25, device="cpu"),
          dict(resolution=ints(2, E.MAX_RES), lo=BOXES, trunc=reals(-1.0, tiny=True)), ["resolution", "lo", "trunc"],
          dict(resolution=1, lo=bad_box, trunc=0.0))

    # -- the surface stage
    sweep(rows, "check_simplify_grid", E.check_simplify_grid, dict(grid=8), dict(grid=ints(2, E.MAX_RES) + vals(0, -1)))
    placements = vals("mean", "quadric", "Mean", "", None, 1, ["mean"], b"mean")
    many = torch.empty((1 << 21) + 1, 3, dtype=torch.float32)
    huge = torch.empty(BIG, 3, dtype=torch.float32)
    big_meshes = [("V = 2^21 + 1", E.Mesh(many, mesh.faces, many)), ("V = 2^24 + 1", E.Mesh(huge, mesh.faces, huge)),
                  ("F = 2^24 + 1", mesh._replace(faces=torch.empty(BIG, 3, dtype=torch.int32)))]
    simp_order = ["grid", "lo", "placement", "mesh"]
    simp_bad = dict(grid=1, lo=bad_box, placement="x", mesh=bad_mesh)
    sweep(rows, "check_simplify_args", E.check_simplify_args, dict(mesh=mesh, grid=512, lo=LO, hi=HI, placement="mean"),
          dict(mesh=mf + big_meshes + [("V = 0", mesh0)], grid=ints(2, E.MAX_RES) + vals(0, -1), lo=BOXES, placement=placements), simp_order, simp_bad)
    rows.append(("check_simplify_args: V = 2^21 + 1 on a coarse grid", E.check_simplify_args, dict(mesh=big_meshes[0][1], grid=64, lo=LO, hi=HI)))
    sweep(rows, "simplify", E.simplify, dict(mesh=mesh, grid=8, lo=LO, hi=HI),
          dict(mesh=mf[:4] + [("V = 0", mesh0), ("no colors", bare)], grid=vals(0, 1, 2.0), placement=placements[2:5]), simp_order, simp_bad)
    smooth_order = ["iterations", "lam", "mu"]
    sweep(rows, "check_smooth_params", E.check_smooth_params, dict(iterations=3, lam=0.5, mu=-0.53),
          dict(iterations=ints(0, E.SMOOTH_MAX_ITERATIONS), lam=reals(1.0, 1.5, -0.1, 1.0 + 1e-9, 0.1, tiny=True),
               mu=reals(-2.0, -2.5, 0.5, -0.1, -2.0 - 1e-9, -1e-50, tiny=True)), smooth_order, dict(iterations=-1, lam="x", mu="y"))
    rows.append(("check_smooth_params: lam out of range + mu not a number", E.check_smooth_params, dict(iterations=1, lam=2.0, mu="y")))
    rows.append(("check_smooth_params: lam out of range + mu out of range", E.check_smooth_params, dict(iterations=1, lam=2.0, mu=1.0)))
    rows.append(("check_smooth_params: defaults", E.check_smooth_params, dict(iterations=0)))
    sm_order = ["iterations", "lam", "mu", "lo", "mesh"]
    sm_bad = dict(iterations=0, lam=2.0, mu=1.0, lo=bad_box, mesh=bad_mesh)
    sweep(rows, "check_smooth_args", E.check_smooth_args, dict(mesh=mesh, iterations=3, lo=LO, hi=HI, lam=0.5, mu=-0.53),
          dict(mesh=mf + big_meshes[1:] + [("V = 0", mesh0)], iterations=ints(1, E.SMOOTH_MAX_ITERATIONS), lo=BOXES, lam=reals(tiny=True), mu=reals()),
          sm_order, sm_bad)
    sweep(rows, "smooth", E.smooth, dict(mesh=mesh, iterations=2, lo=LO, hi=HI),
          dict(mesh=mf[:4] + [("V = 0", mesh0), ("no colors", bare)], iterations=vals(0, True), lam=vals(2.0), mu=vals(0, 1.0)), sm_order, sm_bad)
    rows.append(("_check_mesh_tensors: valid", E._check_mesh_tensors, dict(who="someone", mesh=mesh)))
    for tag, m in mf + big_meshes + [("V = 0", mesh0)]:
        rows.append((f"_check_mesh_tensors: {tag}", E._check_mesh_tensors, dict(who="someone", mesh=m)))

    # -- extract and its callers: the post-processing keywords
    post = dict(min_component=ints(0, 64), largest_only=bools(), opening_radius=ints(0, E.MAX_OPENING_RADIUS),
                simplify_grid=ints(2, E.MAX_RES) + vals(0), simplify_placement=placements[:6],
                smooth_iterations=ints(0, E.SMOOTH_MAX_ITERATIONS), smooth_lambda=reals(tiny=True), smooth_mu=reals())
    post_bad = dict(resolution=1, threshold=math.nan, min_component=-1, largest_only=1, opening_radius=-1, simplify_grid=1, simplify_placement="x",
                    smooth_iterations=-1, smooth_lambda=2.0, smooth_mu=1.0, trunc=0.0, acc_min=0.0, carve=1, min_views=0)
    post_order = ["min_component", "largest_only", "opening_radius", "simplify_grid", "simplify_placement", "smooth_iterations", "smooth_lambda",
                  "smooth_mu"]
    sweep(rows, "extract", E.extract, dict(query=None, activation=E.RELU, resolution=4, threshold=0.5, lo=LO, hi=HI, device="cpu"),
          dict(resolution=ints(2, E.MAX_RES), threshold=reals(), lo=BOXES, **post), ["resolution", "threshold"] + post_order, post_bad)
    sweep(rows, "mesh_volume", E.mesh_volume, dict(query=None, vol=vol, iso=0.5, lo=LO, hi=HI, colors=True),
          dict(vol=volumes, smooth_iterations=post["smooth_iterations"], smooth_lambda=post["smooth_lambda"], smooth_mu=post["smooth_mu"],
               simplify_grid=vals(8)), ["smooth_iterations", "vol"], dict(smooth_iterations=-1, vol=bad_vol))
    sweep(rows, "Trainer.extract_mesh", _trainer_extract, dict(resolution=4, threshold=0.5),
          dict(resolution=ints(2, E.MAX_RES), threshold=reals(), **post), ["resolution", "threshold"] + post_order[:4], post_bad)
    sweep(rows, "Trainer.extract_mesh, on", _trainer_extract, dict(resolution=4, threshold=0.5), {}, ["simplify_grid"] + post_order[5:], post_bad)
    sweep(rows, "NGPTrainer.extract_mesh_tsdf", _trainer_extract_tsdf, dict(resolution=4),
          dict(resolution=ints(2, E.MAX_RES), trunc=reals(), acc_min=reals(), carve=bools(), min_views=ints(1, 1 << 40),
               poses=[("a stack of 17", np.stack([np.eye(4)] * 17)), ("[3, 3]", np.eye(3))], **post),
          ["resolution"] + post_order[:3] + ["trunc", "acc_min", "carve", "min_views"] + post_order[3:], post_bad)

    # -- the texture stage
    rows.append(("texture_layout: valid", E.texture_layout, dict(F=9, texels=8)))
    for Fv, Tv in [(-1, 8), (0, 8), (0, 2), (1 << 24, 2), (BIG, 2), (1 << 24, 8), (9, 1), (9, 2), (9, 64), (9, 65), (-1, 1), (9.0, 8.9), ("9", "8"),
                   (None, 8), (9, None), ("a", 8), (True, True), (123000, 64), (123000, 63)]:
        rows.append((f"texture_layout: F = {Fv!r}, texels = {Tv!r}", E.texture_layout, dict(F=Fv, texels=Tv)))
    wide = mesh._replace(faces=torch.empty(123000, 3, dtype=torch.int32))
    sweep(rows, "check_texture_args", E.check_texture_args, dict(mesh=mesh, texels=8),
          dict(mesh=mf + big_meshes[1:] + [("F = 0", mesh0), ("F = 123000", wide)], texels=ints(2, E.TEXTURE_MAX_TEXELS)),
          ["texels", "mesh"], dict(texels=1, mesh=bad_mesh))
    rows.append(("check_texture_args: F = 123000 at 64 texels", E.check_texture_args, dict(mesh=wide, texels=64)))
    chunks = vals(0, -5, 1, 2.5, 1 << 40, "7", "a", None, True, np.int64(3))
    sweep(rows, "bake_texture", E.bake_texture, dict(query=None, mesh=mesh, texels=T),
          dict(mesh=mf[:3] + [("F = 0", mesh0), ("no colors", bare)], texels=vals(1, 65, True), chunk=chunks), ["texels", "mesh"],
          dict(texels=1, mesh=bad_mesh))
    rows.append(("bake_texture: F = 0 + a bad chunk", E.bake_texture, dict(query=None, mesh=mesh0, texels=T, chunk="a")))
    rows.append(("_check_texture: valid", E._check_texture, dict(who="someone", texture=tex, mesh=mesh)))
    rows.append(("_check_texture: F = 0", E._check_texture, dict(who="someone", texture=tex0, mesh=mesh0)))
    rows.append(("_check_texture: another mesh's", E._check_texture, dict(who="someone", texture=tex0, mesh=mesh)))
    rows.append(("_check_texture: a bad mesh", E._check_texture, dict(who="someone", texture=tex, mesh=bad_mesh)))
    rows.append(("_check_texture: not a Texture + a bad mesh", E._check_texture, dict(who="someone", texture=None, mesh=bad_mesh)))
    rows.append(("_check_texture: texels 1 + a bad mesh", E._check_texture, dict(who="someone", texture=bad_tex, mesh=bad_mesh)))
    for tag, t in tf:
        rows.append((f"_check_texture: {tag}", E._check_texture, dict(who="someone", texture=t, mesh=mesh)))
        rows.append((f"write_obj: {tag}", E.write_obj, dict(path=os.path.join(os.sep, "nonexistent", "directory", "a.obj"), mesh=mesh, texture=t)))
    rows.append(("write_obj: a bad mesh", E.write_obj, dict(path=os.path.join(os.sep, "nonexistent", "directory", "a.obj"), mesh=bad_mesh, texture=tex)))
    face = torch.tensor([0, 1, -1, 5, 1], dtype=torch.int32)
    bary = torch.zeros(5, 2, dtype=torch.float32)
    fb_order, fb_bad = ["face", "bary"], dict(face=face.to(torch.int64), bary=bary[:4])
    sweep(rows, "sample_texture", E.sample_texture, dict(texture=tex, mesh=mesh, face=face, bary=bary),
          dict(texture=tf[:3] + tf[5:7], mesh=mf[:3], face=tfaults(face)[:3] + tfaults(face)[4:], bary=tfaults(bary), rows=vals(True, 1)),
          ["mesh", "texture"] + fb_order, dict(mesh=bad_mesh, texture=tex._replace(image=None), **fb_bad))
    for r in (False, True):
        rows.append((f"sample_texture: n = 0, rows = {r}", E.sample_texture, dict(texture=tex, mesh=mesh, face=face[:0], bary=bary[:0], rows=r)))
    rows.append(("sample_texture: n = 0 and F = 0", E.sample_texture, dict(texture=tex0, mesh=mesh0, face=face[:0], bary=bary[:0])))
    rows.append(("sample_texture: F = 0", E.sample_texture, dict(texture=tex0, mesh=mesh0, face=face, bary=bary)))

    # -- the rasteriser
    raster_order = ["H", "W", "near", "cull_backfaces", "small_max"]
    raster_bad = dict(H=0, W=0, near=0.0, cull_backfaces=1, small_max=-1)
    raster_cases = dict(H=ints(1, E.RASTER_MAX_SIDE), W=ints(1, E.RASTER_MAX_SIDE), near=reals(-0.5, 2, tiny=True), cull_backfaces=bools(),
                        small_max=ints(0, 1 << 30))
    sweep(rows, "check_raster_args", E.check_raster_args, dict(H=48, W=64, near=0.05, cull_backfaces=True, small_max=4), raster_cases, raster_order, raster_bad)
    rows.append(("check_raster_args: defaults", E.check_raster_args, {}))
    cameras = dict(c2w=c2ws[:4] + c2ws[7:13], K=Ks[2:5])
    sweep(rows, "rasterize", E.rasterize, dict(mesh=mesh, c2w=c2w, K=K, H=6, W=5),
          dict(mesh=mf[:3] + [("F = 0", mesh0), ("no colors", bare)], **raster_cases, **cameras), ["mesh"] + raster_order + ["c2w", "K"],
          dict(mesh=bad_mesh, c2w=stack, K=np.eye(2), **raster_bad))
    rows.append(("rasterize: F = 0 + a stack of cameras", E.rasterize, dict(mesh=mesh0, c2w=stack, K=K, H=6, W=5)))
    backgrounds = [("[3]", [0.5, 0.25, 0.0]), ("a tensor [1, 3]", torch.zeros(1, 3)), ("per pixel [30, 3]", torch.zeros(30, 3)),
                   ("per pixel [6, 5, 3]", np.zeros((6, 5, 3))), ("float64 [3]", np.zeros(3)), ("[4]", torch.zeros(4)), ("[3, 30]", torch.zeros(3, 30)),
                   ("[29, 3]", torch.zeros(29, 3)), ("a string", "white"), ("a number", 1.0)]
    render_order = ["mesh"] + raster_order + ["texture", "background", "c2w"]
    sweep(rows, "render_mesh", E.render_mesh, dict(mesh=mesh, c2w=c2w, K=K, H=6, W=5),
          dict(mesh=mf[:3] + [("F = 0", mesh0), ("no colors", bare)], texture=[("one", tex)] + tf[:3] + tf[5:7], background=backgrounds, **raster_cases,
               **cameras), render_order, dict(mesh=bad_mesh, texture=bad_tex, background=torch.zeros(4), c2w=stack, **raster_bad))
    for tag, kw in [("no colors + a bad background", dict(mesh=bare, background="white")), ("no colors + a texture", dict(mesh=bare, texture=tex)),
                    ("no colors + bad small_max", dict(mesh=bare, small_max=-1)), ("F = 0 + a texture", dict(mesh=mesh0, texture=tex0)),
                    ("F = 0 + a background per pixel", dict(mesh=mesh0, background=torch.zeros(30, 3))),
                    ("F = 0 + one background", dict(mesh=mesh0, background=[0.5, 0.25, 0.0])),
                    ("F = 0 + a bad background + a stack of cameras", dict(mesh=mesh0, background="white", c2w=stack)),
                    ("F = 0 + a stack of cameras", dict(mesh=mesh0, c2w=stack)), ("F = 0, no colors", dict(mesh=mesh0._replace(colors=None)))]:
        rows.append((f"render_mesh: {tag}", E.render_mesh, dict(dict(mesh=mesh, c2w=c2w, K=K, H=6, W=5), **kw)))

    # -- the mip pyramid
    for t in [True, 2.0, np.int64(8), np.int32(4), 1, 2, 3, 4, 5, 8, 9, 33, 63, 64, 65, 0, -1, "8", None]:
        rows.append((f"mip_levels: texels = {t!r}", E.mip_levels, dict(texels=t)))
    sweep(rows, "build_mipmaps", E.build_mipmaps, dict(texture=tex, mesh=mesh),
          dict(texture=tf + [("one level", tex2), ("F = 0", tex0)], mesh=mf[:3] + [("F = 0", mesh0)], chunk=chunks), ["mesh", "texture"],
          dict(mesh=bad_mesh, texture=tex._replace(image=None)))
    rows.append(("build_mipmaps: F = 0", E.build_mipmaps, dict(texture=tex0, mesh=mesh0)))
    rows.append(("build_mipmaps: F = 0 + a bad chunk", E.build_mipmaps, dict(texture=tex0, mesh=mesh0, chunk="a")))
    rows.append(("build_mipmaps: one level + a bad chunk", E.build_mipmaps, dict(texture=tex2, mesh=mesh, chunk="a")))
    rows.append(("_check_pyramid: valid", E._check_pyramid, dict(who="someone", pyramid=pyr, mesh=mesh)))
    rows.append(("_check_pyramid: F = 0", E._check_pyramid, dict(who="someone", pyramid=pyr0, mesh=mesh0)))
    rows.append(("_check_pyramid: one level", E._check_pyramid, dict(who="someone", pyramid=E.TexturePyramid((tex2,)), mesh=mesh)))
    rows.append(("_check_pyramid: a bad mesh", E._check_pyramid, dict(who="someone", pyramid=pyr, mesh=bad_mesh)))
    for tag, p in pf:
        rows.append((f"_check_pyramid: {tag}", E._check_pyramid, dict(who="someone", pyramid=p, mesh=mesh)))
    sweep(rows, "check_lod_scale", E.check_lod_scale, dict(scale=1.5), dict(scale=reals(-1.0, 2, tiny=True)))
    sweep(rows, "face_lod", E.face_lod, dict(mesh=mesh, c2w=c2w, K=K),
          dict(mesh=mf[:3] + [("F = 0", mesh0)], near=reals(tiny=True), texels=ints(2, E.TEXTURE_MAX_TEXELS), scale=reals(tiny=True), **cameras),
          ["mesh", "near", "texels", "scale", "c2w", "K"], dict(mesh=bad_mesh, near=0.0, texels=1, scale=0.0, c2w=stack, K=np.eye(2)))
    rows.append(("face_lod: F = 0 + a stack of cameras", E.face_lod, dict(mesh=mesh0, c2w=stack, K=K)))
    lod, lod_f = torch.zeros(5, dtype=torch.float32), torch.zeros(F, dtype=torch.float32)
    sweep(rows, "sample_texture_mip", E.sample_texture_mip, dict(pyramid=pyr, mesh=mesh, face=face, bary=bary, lod=lod),
          dict(pyramid=pf, mesh=mf[:3], per_face=bools(), face=tfaults(face)[:3] + tfaults(face)[4:], bary=tfaults(bary), lod=tfaults(lod) + [("per face", lod_f)]),
          ["mesh", "pyramid", "per_face"] + fb_order + ["lod"], dict(mesh=bad_mesh, pyramid=bad_pyr, per_face=1, lod=lod[:4], **fb_bad))
    per_face = dict(pyramid=pyr, mesh=mesh, face=face, bary=bary, lod=lod_f, per_face=True)
    rows.append(("sample_texture_mip: per face", E.sample_texture_mip, per_face))
    for tag, bad in tfaults(lod_f) + [("per sample", lod)]:
        rows.append((f"sample_texture_mip: per face, lod {tag}", E.sample_texture_mip, dict(per_face, lod=bad)))
    rows.append(("sample_texture_mip: n = 0", E.sample_texture_mip, dict(pyramid=pyr, mesh=mesh, face=face[:0], bary=bary[:0], lod=lod[:0])))
    rows.append(("sample_texture_mip: n = 0, per face", E.sample_texture_mip, dict(per_face, face=face[:0], bary=bary[:0])))
    rows.append(("sample_texture_mip: F = 0", E.sample_texture_mip, dict(pyramid=pyr0, mesh=mesh0, face=face, bary=bary, lod=lod)))
    rows.append(("sample_texture_mip: F = 0, per face", E.sample_texture_mip, dict(pyramid=pyr0, mesh=mesh0, face=face, bary=bary, lod=lod[:0], per_face=True)))
    mip_order = ["mesh"] + raster_order + ["pyramid", "lod_scale", "background", "c2w"]
    sweep(rows, "render_mesh_mip", E.render_mesh_mip, dict(mesh=mesh, c2w=c2w, K=K, H=6, W=5, pyramid=pyr),
          dict(mesh=mf[:3] + [("F = 0", mesh0), ("no colors", bare)], pyramid=pf[:6], lod_scale=reals(tiny=True), background=backgrounds, **raster_cases,
               **cameras), mip_order, dict(mesh=bad_mesh, pyramid=bad_pyr, lod_scale=0.0, background=torch.zeros(4), c2w=stack, **raster_bad))
    for tag, kw in [("F = 0", {}), ("F = 0 + a background per pixel", dict(background=torch.zeros(30, 3))), ("F = 0 + a stack of cameras", dict(c2w=stack)),
                    ("F = 0 + a bad background + a stack of cameras", dict(background="white", c2w=stack))]:
        rows.append((f"render_mesh_mip: {tag}", E.render_mesh_mip, dict(dict(mesh=mesh0, c2w=c2w, K=K, H=6, W=5, pyramid=pyr0), **kw)))

    # -- the projective bake
    proj_order = ["depth_tol", "mode", "near", "cos_min", "acc_min", "chunk"]
    proj_bad = dict(depth_tol=-1.0, mode="x", near=0.0, cos_min=0.0, acc_min=0.0, chunk=0)
    proj_cases = dict(depth_tol=reals(-1.0, 2, float(np.finfo(np.float32).max), 3.5e38, tiny=True), mode=vals("blend", "best", "Blend", None, 0, ["best"]),
                      near=reals(tiny=True), cos_min=reals(1.0, 1.5, 1.0 + 1e-9, tiny=True), acc_min=reals(1.0, 1.5, tiny=True), chunk=ints(1, 1 << 40))
    sweep(rows, "check_project_args", E.check_project_args, dict(depth_tol=0.01, mode="best", near=0.05, cos_min=0.1, acc_min=0.5, chunk=100),
          proj_cases, proj_order, proj_bad)
    rows.append(("check_project_args: defaults", E.check_project_args, dict(depth_tol=0)))
    images = torch.zeros(2, 6, 5, 3, dtype=torch.float32)
    maps = torch.zeros(2, 6, 5, dtype=torch.float32)
    image_cases = [(t, v) for t, v in tfaults(images) if t != "rows"] + \
        [("RGBA", torch.zeros(2, 6, 5, 4)), ("RGBA float64", torch.zeros(2, 6, 5, 4, dtype=torch.float64)), ("RGBA [6, 5, 4]", torch.zeros(6, 5, 4)),
         ("one view", images[:1]), ("three views", torch.zeros(3, 6, 5, 3)), ("n = 0", images[:0]), ("W = 16385", torch.zeros(1, 1, 16385, 3)),
         ("H = 0", torch.zeros(2, 0, 5, 3))]
    map_cases = [(t, v) for t, v in tfaults(maps) if t != "rank"] + [("flat", maps.reshape(-1)), ("[2, 30]", maps.reshape(2, 30)), ("None", None)]
    fallbacks = [("one", tex)] + tf + [("F = 0's", tex0)]
    base = dict(mesh=mesh, images=images, c2w=stack, K=K, texels=T, depth_tol=0.01)
    sweep(rows, "project_texture", E.project_texture, base,
          dict(mesh=mf[:3] + [("F = 0", mesh0), ("no colors", bare)], images=image_cases, c2w=c2ws[:4] + c2ws[7:13], K=Ks[2:5], texels=ints(2, E.TEXTURE_MAX_TEXELS),
               fallback=fallbacks, **proj_cases),
          ["texels", "mesh"] + proj_order + ["images", "c2w"], dict(texels=1, mesh=bad_mesh, images=images.to(torch.float64), c2w=c2w, **proj_bad))
    both = dict(base, depth=maps, acc=maps.clone())
    sweep(rows, "project_texture with maps", E.project_texture, both, dict(depth=map_cases, acc=map_cases, fallback=fallbacks),
          ["c2w", "depth", "acc", "fallback"], dict(c2w=c2w, depth=maps.to(torch.float64), acc=maps[:1], fallback=bad_tex))
    for tag, kw in [("W = 16385 + one pose too many", dict(images=torch.zeros(1, 1, 16385, 3))), ("bad images + W = 16385", dict(images=torch.zeros(1, 1, 16385, 4))),
                    ("one pose too many + depth alone", dict(c2w=c2w, depth=maps)), ("depth alone + a bad depth", dict(depth=maps[:1])),
                    ("acc alone + a bad fallback", dict(acc=maps, fallback=bad_tex)), ("n = 0", dict(images=images[:0], c2w=None)),
                    ("n = 0 with maps", dict(images=images[:0], c2w=None, depth=maps[:0], acc=maps[:0])),
                    ("n = 0 + a bad K", dict(images=images[:0], K=None)), ("F = 0", dict(mesh=mesh0)), ("F = 0 with a fallback", dict(mesh=mesh0, fallback=tex0)),
                    ("F = 0 with another mesh's fallback", dict(mesh=mesh0, fallback=tex)), ("F = 0, n = 0", dict(mesh=mesh0, images=images[:0], c2w=None)),
                    ("F = 0 + one pose too many", dict(mesh=mesh0, c2w=c2w)), ("a fallback of other texels", dict(fallback=tex2)),
                    ("a bad chunk", dict(chunk=2.5))]:
        rows.append((f"project_texture: {tag}", E.project_texture, dict(base, **kw)))
    seen = {}
    for k, (label, fn, kw) in enumerate(rows):                  # (two values of a parameter may print alike)
        seen[label] = seen.get(label, 0) + 1
        if seen[label] > 1:
            rows[k] = (f"{label} #{seen[label]}", fn, kw)
    return rows


# ------------------------------------------------------------------------------------------------ the recording
def _norm(x):
    if isinstance(x, torch.Tensor):
        return f"tensor {str(x.dtype)[6:]} {list(x.shape)} {x.device.type}"
    if isinstance(x, np.ndarray):
        return ["ndarray", str(x.dtype), list(x.shape), [repr(float(v)) for v in x.ravel()]]
    if x is None or isinstance(x, (bool, int, str)):
        return x
    if isinstance(x, float):
        return repr(x)
    if isinstance(x, np.generic):
        return [type(x).__name__, repr(x.item())]
    if isinstance(x, (tuple, list)):
        return [type(x).__name__] + [_norm(v) for v in x]
    if isinstance(x, E.TSDFVolume):
        return ["TSDFVolume", x.R, _norm(x.lo), _norm(x.hi), _norm(x.trunc)]
    raise TypeError(f"a result of type {type(x).__name__}")


def outcome(fn, kw):
    """'<exception type>: <text>' of a refusal, or '= <the result>' of a return."""
    try:
        with np.errstate(all="ignore"):
            got = fn(**kw)
    except Exception as e:                                      # noqa: BLE001  (which exception it is, is what is recorded)
        return f"{type(e).__name__}: {e}"
    return "= " + json.dumps(_norm(got))


def record():
    return [[label, outcome(fn, kw)] for label, fn, kw in table()]


def compact(rec):
    """The file form: every distinct outcome once, the calls as indices into them, no labels."""
    texts = sorted({o for _, o in rec})
    return {"texts": texts, "calls": [texts.index(o) for _, o in rec]}


def expand(data, labels):
    assert len(data["calls"]) == len(labels), "the recording holds another list of calls than table() makes"
    return [[label, data["texts"][i]] for label, i in zip(labels, data["calls"])]


@pytest.fixture(scope="module")
def got():
    return record()


@pytest.fixture(scope="module")
def want(got):
    with open(GOLDEN) as f:
        return expand(json.load(f), [label for label, _ in got])


def test_every_call_ends_as_recorded(got, want):
    """Nothing is skipped: every call of the table is made and compared."""
    assert len(got) == len(want) > 2000 and len({label for label, _ in got}) == len(got)
    diff = [(label, a, b) for (label, a), (_, b) in zip(got, want) if a != b]
    assert not diff, (len(diff), diff[:8])


def test_the_recording_holds_refusals_and_pure_returns_only(want):
    kinds = {}
    for label, text in want:
        kind = "=" if text.startswith("= ") else text.split(":", 1)[0]
        kinds.setdefault(kind, []).append(label)
    # ValueError: a refusal, the library's among them, or _native.ptr's; TypeError and AttributeError: Python's own, of float(None), len(None) or a
    # tuple that has no fields, which the layer lets through as they are
    assert set(kinds) == {"=", "ValueError", "TypeError", "AttributeError"}, {k: v[:3] for k, v in kinds.items() if k not in ("=", "ValueError")}
    assert len(kinds["TypeError"]) + len(kinds["AttributeError"]) < len(want) // 10
    by = dict(want)
    launched = {label for label, text in want if text == NO_CPU_PATH}
    for fn in ("marching_cubes", "connected_components", "filter_components", "erode", "reconstruct", "open_components", "TSDFVolume", "simplify",
               "smooth", "bake_texture", "sample_texture", "rasterize", "render_mesh", "build_mipmaps", "face_lod", "sample_texture_mip",
               "render_mesh_mip", "project_texture", "project_texture with maps", "extract", "mesh_volume", "Trainer.extract_mesh",
               "NGPTrainer.extract_mesh_tsdf", "density_volume"):
        assert f"{fn}: valid" in launched, fn
    for fn in ("check_mesh_args", "check_component_args", "check_opening_args", "check_tsdf_args", "check_simplify_grid", "check_simplify_args",
               "check_smooth_params", "check_smooth_args", "check_texture_args", "check_raster_args", "check_lod_scale", "check_project_args",
               "tsdf_views", "texture_layout", "_check_mesh_tensors", "_check_texture", "_check_pyramid"):
        assert by[f"{fn}: valid"].startswith("= "), fn
        assert not any(label.startswith(fn + ":") for label in launched), fn
    # the irregular texts are in it
    texts = set(by.values())
    for t in ("ValueError: tsdf H must be an int in [1, 2^24], got 0", "ValueError: simplify_grid must be 0 or an int in [2, 512], got 1",
              "ValueError: tsdf min_views must be an int >= 1, got 0", "ValueError: smooth lambda must be in (0, 1] as a float32, got 0.0",
              "ValueError: someone: faces must be a contiguous int32 [F, 3] tensor on the vertices' device",
              "ValueError: project_texture: images must be a contiguous float32 [n, H, W, 3] tensor on the vertices' device (RGBA frames are not supported)",
              "ValueError: someone: need an engine.mesh.Mesh, got tuple", "ValueError: project chunk must be an int >= 1, got 0",
              "ValueError: raster small_max must be an int in [0, 2^30], got -1"):
        assert t in texts, t
    assert by["check_smooth_params: mu = -1e-50"] == '= ["tuple", 3, "0.5", "-0.0"]'
    assert by["render_mesh: mesh = F = 0"].startswith('= ["MeshFrame", "tensor float32 [6, 5, 3] cpu"')


if __name__ == "__main__":
    json.dump(compact(record()), sys.stdout, separators=(",", ":"))
