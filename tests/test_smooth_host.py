"""Mesh smoothing without a GPU: properties of the numpy reference (tests/_smooth_ref.py) of include/nerf_hip.h "mesh smoothing"
on noisy marching-cubes spheres, the argument checks of engine.mesh, the header / binding / pipeline bookkeeping, and the workspace
carve of csrc/smooth_ws.h in a stand-alone program built with the host compiler and -fsanitize=address,undefined
(tests/smooth_ws_check.cpp).  The GPU side is held to this reference bit for bit in tests/test_gpu_smooth.py."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import _mesh_ref as M
from tests import _smooth_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ reference properties
@pytest.mark.parametrize("R,sizes", [(12, (386, 768)), (24, (2074, 4064))])
def test_taubin_halves_the_roughness_and_keeps_the_volume(R, sizes):
    """10 pairs at (0.5, -0.53).  Measured with these constants: roughness x0.33 / x0.32; enclosed volume +1.5 % / -0.5 % for
    Taubin against -28 % / -7.7 % for plain Laplacian."""
    v, f = S.sphere(R)
    assert (len(v), len(f)) == sizes and M.closed_and_oriented(f)
    vt, nt = S.smooth(v, f, 10, S.LO, S.HI)
    vl, _ = S.smooth(v, f, 10, S.LO, S.HI, S.LAM, 0.0)
    assert S.roughness(vt, f) < 0.5 * S.roughness(v, f)
    vol = M.enclosed_volume(v, f)
    dt, dl = abs(M.enclosed_volume(vt, f) / vol - 1.0), abs(M.enclosed_volume(vl, f) / vol - 1.0)
    assert dt < 0.25 * dl, (dt, dl)
    # the normals of the result: the normalised sums of the face normals (v_b - v_a) x (v_c - v_a) of plain float64 numpy
    x = vt.astype(np.float64)
    fn = np.cross(x[f[:, 1]] - x[f[:, 0]], x[f[:, 2]] - x[f[:, 0]])
    want = np.zeros_like(x)
    for c in range(3):
        np.add.at(want, f[:, c], fn)
    want /= np.linalg.norm(want, axis=1, keepdims=True)
    assert np.abs(nt.astype(np.float64) - want).max() < 1e-6


# ------------------------------------------------------------------------------------------------ reference invariances
def test_face_order_changes_no_bit():
    v, f = S.sphere(12)
    want = S.smooth(v, f, 3, S.LO, S.HI)
    got = S.smooth(v, f[np.random.default_rng(0).permutation(len(f))], 3, S.LO, S.HI)
    assert np.array_equal(_bits(want[0]), _bits(got[0])) and np.array_equal(_bits(want[1]), _bits(got[1]))


def test_vertex_renumbering_permutes_the_bits():
    v, f = S.sphere(12)
    perm = np.random.default_rng(1).permutation(len(v))              # new index of old vertex i
    v2 = np.empty_like(v)
    v2[perm] = v
    f2 = perm[f].astype(np.int32)
    want = S.smooth(v, f, 3, S.LO, S.HI)
    got = S.smooth(v2, f2, 3, S.LO, S.HI)
    assert np.array_equal(_bits(want[0]), _bits(got[0][perm])) and np.array_equal(_bits(want[1]), _bits(got[1][perm]))


def test_ignored_faces_a_nan_vertex_and_an_unreferenced_vertex():
    v, f, i_nan, i_free = S.junk(12)
    v0, f0 = S.sphere(12)
    assert len(f) == len(f0) + 8 and len(v) == len(v0) + 1
    clean_v = v.copy()
    got = S.smooth(v, f, 4, S.LO, S.HI)
    want = S.smooth(clean_v, f0, 4, S.LO, S.HI)                       # the same vertices without the appended faces
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[1]), _bits(want[1]))
    assert np.array_equal(_bits(got[0][i_nan]), _bits(v[i_nan]))      # returned bit for bit, NaN included
    others = np.delete(np.arange(len(v)), i_nan)
    assert np.isfinite(got[0][others]).all() and np.isfinite(got[1]).all()
    nb = np.unique(f0[(f0 == i_nan).any(1)])
    nb = nb[nb != i_nan]
    assert len(nb) >= 3 and not np.array_equal(_bits(got[0][nb]), _bits(v[nb]))     # its neighbours still move
    assert np.array_equal(_bits(got[0][i_free]), _bits(v[i_free])) and not got[1][i_free].any()
    assert not got[1][i_nan].any()


def test_interior_of_a_flat_regular_patch_stays():
    """Two pairs = four half-steps: the boundary's pull reaches ring 3; rings 4 and 5 of an 11 x 11 sheet see only symmetric
    umbrellas of unmoved neighbours, so they move by rounding alone."""
    v, f = S.grid_mesh(11, 11, flat=True)
    out, nrm = S.smooth(v, f, 2, S.LO, S.HI)
    i, j = np.meshgrid(np.arange(11), np.arange(11), indexing="ij")
    ring = np.minimum(np.minimum(i, 10 - i), np.minimum(j, 10 - j)).ravel()
    inner = ring >= 4
    assert inner.sum() == 9
    ulp = np.spacing(np.abs(v[inner]).astype(np.float32))
    assert (np.abs(out[inner].astype(np.float64) - v[inner]) <= 4 * ulp).all()
    assert not np.array_equal(out[ring == 0], v[ring == 0])
    assert np.allclose(nrm[inner], [0.0, 0.0, 1.0], atol=1e-6)


def test_boundary_weights_and_the_written_half_step():
    """One half-step on a single triangle by hand: every neighbour has weight 1, the mean is the other two corners' midpoint."""
    v = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 1.0], [0.0, 1.0, 1.0]], np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    ctr, ext = S.box(S.LO, S.HI)
    out = S.half_step(v, S.entries(f, 3), ctr, ext, 0.5)
    assert np.allclose(out, [[0.25, 0.25, 1.0], [0.5, 0.25, 1.0], [0.25, 0.5, 1.0]], atol=1e-7)
    assert np.array_equal(S.normals(v, S.entries(f, 3), ctr, ext), np.array([[0, 0, 1]] * 3, np.float32))


def test_fixed_point_constants_meet_the_header_bounds():
    assert 2 ** 25 * S.POS_LIM * S.POS_SCALE < 2 ** 63 and 1.0 / S.POS_SCALE <= 2.0 ** -30
    assert 2 ** 24 * S.NRM_LIM * S.NRM_SCALE < 2 ** 63 and 512.0 ** -2 * S.NRM_SCALE >= 2 ** 16


# ------------------------------------------------------------------------------------------------ host-side API
def test_argument_checks():
    from nerf_meets_mlx_amd.engine import mesh as E
    v, f = (torch.from_numpy(a.copy()) for a in S.sphere(12))
    n = torch.zeros_like(v)
    good = E.Mesh(v, f, n, None)
    assert E.check_smooth_args(good, 10, S.LO, S.HI) == (10, S.LO, S.HI, 0.5, float(np.float32(-0.53)))
    assert E.check_smooth_args(good._replace(colors=n), 1, S.LO, S.HI, 1.0, 0.0)[3:] == (1.0, 0.0)
    assert E.check_smooth_args(good, E.SMOOTH_MAX_ITERATIONS, S.LO, S.HI, np.float32(0.25), -2)[3:] == (0.25, -2.0)
    for it in (0, -1, E.SMOOTH_MAX_ITERATIONS + 1, 3.0, True, None, "3"):
        with pytest.raises(ValueError):
            E.check_smooth_args(good, it, S.LO, S.HI)
    for lam in (0.0, -0.5, 1.5, float("nan"), 1e-60, True, None, "0.5"):
        with pytest.raises(ValueError):
            E.check_smooth_args(good, 3, S.LO, S.HI, lam)
    for mu in (0.1, -2.5, float("nan"), float("-inf"), False, None, "-0.5"):
        with pytest.raises(ValueError):
            E.check_smooth_args(good, 3, S.LO, S.HI, 0.5, mu)
    for lo, hi in (([0.0] * 3, [0.0] * 3), ([-1, -1, 1], [1, 1, 1]), ([-1, -1], [1, 1]), ([-1, -1, float("nan")], [1, 1, 1])):
        with pytest.raises(ValueError):
            E.check_smooth_args(good, 3, lo, hi)
    bad = [good._replace(verts=v.double()), good._replace(faces=f.long()), good._replace(normals=n[:-1]),
           good._replace(colors=n[:, :2]), good._replace(verts=v.t().contiguous().t()), good._replace(faces=f[:, :2]),
           good._replace(normals=None), good._replace(verts=v.numpy()), (v, f)]
    for m in bad:
        with pytest.raises(ValueError):
            E.check_smooth_args(m, 3, S.LO, S.HI)
    assert E.check_smooth_params(0) == (0, 0.5, float(np.float32(-0.53)))
    with pytest.raises(ValueError):
        E.check_smooth_params(-1)


def test_header_section_bindings_and_makefile():
    from nerf_meets_mlx_amd import _native
    text = open(os.path.join(ROOT, "include", "nerf_hip.h")).read()
    start = text.index("mesh smoothing (no reference counterpart)")
    assert text.index("mesh simplification (no reference counterpart)") < start
    section = text[start:text.index("/* ----", start)]
    decl = re.sub(r"/\*.*?\*/", "", "/*" + section, flags=re.S)
    entries = sorted(set(re.findall(r"\b(nerf_smooth_[a-z_]+)\s*\(", decl)))
    assert entries == ["nerf_smooth_build", "nerf_smooth_normals", "nerf_smooth_run", "nerf_smooth_workspace_bytes"]
    for e in entries:
        assert e in _native.SIGNATURES
    for word in ("fix(u_x, 4, 2^32)", "fix(c_x, 16, 2^34)", "Not done", "cotangent", "bilateral"):
        assert word in section
    assert "#define NERF_ABI_VERSION 3" in text
    mk = open(os.path.join(ROOT, "nerf_meets_mlx_amd", "csrc", "Makefile")).read()
    srcs = next(ln for ln in mk.splitlines() if ln.startswith("SRCS"))
    assert "smooth.hip" in srcs.split() and "smooth_ws.h" in mk
    src = open(os.path.join(ROOT, "nerf_meets_mlx_amd", "csrc", "smooth.hip")).read()
    kernels = sorted(set(re.findall(r"\b(\w+_kernel)\(", src)))
    assert kernels == ["smooth_count_kernel", "smooth_fill_kernel", "smooth_normals_kernel", "smooth_step_kernel"]
    # the row offsets are csrc/scan.h's counts-to-offsets pair, defined there once and launched here: six kernels as before
    scan = open(os.path.join(ROOT, "nerf_meets_mlx_amd", "csrc", "scan.h")).read()
    for name in ("scan_offsets_count_kernel", "scan_offsets_write_kernel"):
        assert len(re.findall(r"\b" + name + r"\(", scan)) == 1 and src.count(name + "<SMOOTH_BLOCK>,") == 1, name


def test_pipeline_keywords_and_defaults():
    from nerf_meets_mlx_amd.engine import mesh as E
    from nerf_meets_mlx_amd.engine.ngp import NGPTrainer
    from nerf_meets_mlx_amd.engine.trainer import Trainer
    want = [("smooth_iterations", 0), ("smooth_lambda", 0.5), ("smooth_mu", -0.53)]
    for fn in (E.extract, E.mesh_volume, Trainer.extract_mesh, NGPTrainer.extract_mesh_tsdf):
        p = list(inspect.signature(fn).parameters.values())
        assert [(q.name, q.default) for q in p[-3:]] == want, fn.__qualname__       # appended: positional callers are unaffected
        assert [q.name for q in p[-5:-3]] == ["simplify_grid", "simplify_placement"]
    p = inspect.signature(E.smooth).parameters
    assert list(p) == ["mesh", "iterations", "lo", "hi", "lam", "mu"] and (p["lam"].default, p["mu"].default) == (0.5, -0.53)


def test_mesh_tool_stats_know_the_smoother_kernels(tmp_path, capsys):
    import argparse
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("ngp_mesh_tool", os.path.join(ROOT, "tools", "ngp_mesh.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    src = open(os.path.join(ROOT, "nerf_meets_mlx_amd", "csrc", "smooth.hip")).read()
    kernels = sorted(set(re.findall(r"\b(smooth_\w+_kernel)\(", src)))
    path = tmp_path / "trace.csv"
    with open(path, "w") as fh:
        fh.write('"Kernel_Name","Start_Timestamp","End_Timestamp","Grid_Size_X"\n')
        for i, k in enumerate(kernels):
            for rep in range(2):
                fh.write(f'"void nerf::(anonymous namespace)::{k}(float const*, int)",{1000 * i},{1000 * i + 500 + 1000 * rep},{256 * (i + 1)}\n')
    tool.stats(argparse.Namespace(stats=str(path), from_=None, out=None))
    recs = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert sorted(r["kernel"] for r in recs) == kernels
    assert all(r["launches"] == 2 and r["avg_us"] == 1.0 for r in recs)
    args = tool.parser().parse_args(["--smooth", "5", "--smooth", "10"])
    assert args.smooth == [5, 10] and (args.smooth_lambda, args.smooth_mu) == (0.5, -0.53)
    assert tool.parser().parse_args([]).smooth is None


# ------------------------------------------------------------------------------------------------ workspace carve
SIZES = [(0, 0), (1, 1), (4, 4), (257, 511), (1 << 24, 1 << 24)]


@pytest.fixture(scope="module")
def carved(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("smooth_ws") / "smooth_ws_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "smooth_ws_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    ws, bad, cur = {}, None, None
    for ln in out.stdout.splitlines():
        w = ln.split()
        if w[0] == "ws":
            cur = ws[(int(w[1]), int(w[2]))] = {"bytes": int(w[4]), "total": int(w[6]), "nblk": int(w[8]), "regions": {}}
        elif w[0] == "region":
            cur["regions"][w[1]] = (int(w[2]), int(w[3]))
        elif w[0] == "same":
            cur["same"] = int(w[1])
        elif w[0] == "bad":
            bad = [int(x) for x in w[1:]]
        elif w[0] == "entry":
            assert int(w[1]) == 8
    return ws, bad


@pytest.mark.parametrize("V,F", SIZES)
def test_workspace_regions_are_disjoint_aligned_and_complete(carved, V, F):
    got = carved[0][(V, F)]
    assert got["bytes"] == got["total"] and got["nblk"] == -(-V // 256) and got["same"] == 1
    r = got["regions"]
    assert sorted(r) == ["blk", "cur", "ent", "off", "tmp", "total"]
    assert r["blk"][1] == 8 * got["nblk"] and r["tmp"][1] == 12 * V and r["off"][1] == 4 * (V + 1) and r["cur"][1] == 4 * V
    assert r["ent"][1] == 24 * F and r["total"][1] == 8
    spans = sorted(r.values())
    assert spans[0][0] == 0
    for (a, n), (b, _) in zip(spans, spans[1:]):
        assert a + n <= b < a + n + 8                              # disjoint, and only alignment padding between
    assert all(a % 8 == 0 for a, _ in spans)
    last = max(a + n for a, n in spans)
    assert last <= got["bytes"] < last + 8 and got["bytes"] % 8 == 0
    assert max(r, key=lambda k: (r[k][0], k == "ent")) == "ent"    # last: the only region whose size depends on F


def test_workspace_sizes_out_of_range(carved):
    assert carved[1] == [-1] * 5
