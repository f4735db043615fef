"""csrc/camera.h and the mesh arguments of csrc/lattice.h on the host.  (1) The host layer of every entry that takes a camera, an
image size or a mesh (TSDF fusion, the rasteriser, the projective bake, the mip pyramid, the texture atlas) against a recording of
itself from before their checks were folded onto those two headers: (return code, error text) of calls that return before any
launch, every fault alone, every pair of faults in two different arguments (which check wins is part of the behaviour) and the
`nothing to do` calls.  `python -m tests.test_camera_host` with NERF_HIP_LIB=<the library of the parent commit> wrote
tests/golden/camera_parent.json; the tests make the same calls on the library under test.  (2) The camera itself, bit for bit: a
stand-alone program (tests/camera_check.cpp) built with the host compiler and -fsanitize=address,undefined prints camera_point,
camera_pixel and camera_nearest for two cameras and about 1000 points each, and the return codes of the checks; the floats are compared
as bit patterns with tests/_camera_ref.py, on which the TSDF, raster and bake references are built.  No GPU."""
import ctypes as C
import itertools
import json
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from nerf_meets_mlx_amd import _native as N
from tests import _camera_ref as CR
from tests.test_compaction_host import compact, expand

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "camera_parent.json")
NERF_OK, NERF_E_NULL, NERF_E_SHAPE = 0, -1, -2

P = C.c_void_p(4096)                                # non-NULL, 16-byte aligned, never dereferenced: no call below reaches a launch
ODD = C.c_void_p(4100)                              # not 16-byte aligned
LO, HI = (C.c_float * 3)(-1.0, -1.0, -1.0), (C.c_float * 3)(1.0, 1.0, 1.0)
HI_NAN = (C.c_float * 3)(1.0, math.nan, 1.0)
BIG = (1 << 24) + 1
NVIEWS = 3


def _views(n, bad_view=-1, bad_number=0, bad_value=math.nan):
    x = [0.25 * (q + 1) + s for s in range(n) for q in range(16)]
    if bad_view >= 0:
        x[16 * bad_view + bad_number] = bad_value
    return (C.c_float * (16 * n))(*x)


def _number_faults(pos, views):
    """Each of the 16 camera numbers not finite, in the first and in the last of `views` views, at argument `pos`."""
    return {f"view {s} number {q} {'nan' if q % 2 else 'inf'}": (pos, _views(views, s, q, math.nan if q % 2 else math.inf))
            for s in sorted({0, views - 1}) for q in range(16)}


def _side_faults(h, w, bound):
    return {"H 0": (h, 0), "W 0": (w, 0), f"H {bound + 1}": (h, bound + 1), f"W {bound + 1}": (w, bound + 1), "H -3": (h, -3), "W -3": (w, -3)}


def _near_faults(pos):
    return {"near 0": (pos, 0.0), "near nan": (pos, math.nan), "near inf": (pos, math.inf)}


def _mesh_faults(v, f):
    out = {"F -1": (f, -1), "F 2^24 + 1": (f, BIG)}
    if v is not None:
        out.update({"V -1": (v, -1), "V 2^24 + 1": (v, BIG)})
    return out


def _nulls(**pos):
    return {f"NULL {k}": (p, None) for k, p in pos.items()}


LEVELS = (C.c_void_p * 6)(*([4096] * 6))
LEVELS_HOLE = (C.c_void_p * 6)(4096, None, 4096, 4096, 4096, 4096)
CHUNK = {"p0 -1": (0, -1), "count -1": (1, -1), "chunk past the end": (0, 598)}           # 9 faces at T = 8: an atlas of 30 x 20 texels


def _chunk(p0):
    return {k: (p0 + d, v) for k, (d, v) in CHUNK.items()}


TEXELS = {"texels 1": 1, "texels 65": 65}

# entry -> (valid arguments: a launch, so never called as they are; faults as {name: (position, value)})
ENTRIES = {
    "nerf_tsdf_integrate": ([P, P, P, 65, LO, HI, _views(NVIEWS), NVIEWS, 48, 64, P, P, 0.1, 0.5, 6.0, 1, None],
                            dict(_side_faults(8, 9, 1 << 24), **_number_faults(6, NVIEWS),
                                 **_nulls(D=0, Wt=1, flags=2, lo=4, hi=5, views=6, depth=10, acc=11),
                                 **{"res 1": (3, 1), "res 513": (3, 513), "hi nan": (5, HI_NAN), "n -1": (7, -1), "n 17": (7, 17),
                                    "trunc 0": (12, 0.0), "trunc nan": (12, math.nan), "acc_min 0": (13, 0.0), "acc_min 1.5": (13, 1.5),
                                    "far 0": (14, 0.0), "far inf": (14, math.inf), "carve 2": (15, 2)})),
    "nerf_raster_clear": ([P, 48, 64, P, None], dict(_side_faults(1, 2, 16384), **_nulls(keys=0, stats=3))),
    "nerf_raster_draw": ([P, 10, P, 9, 0, _views(1), 48, 64, 0.05, 1, 16, P, P, None],
                         dict(_side_faults(6, 7, 16384), **_mesh_faults(1, 3), **_near_faults(8), **_number_faults(5, 1),
                              **_nulls(verts=0, faces=2, view=5, keys=11, stats=12),
                              **{"face_base -1": (4, -1), "face_base 2^24": (4, 1 << 24), "cull 2": (9, 2), "small_max -1": (10, -1),
                                 "small_max 2^30 + 1": (10, (1 << 30) + 1)})),
    "nerf_raster_resolve": ([P, P, 10, P, 9, _views(1), 48, 64, 0.05, P, P, P, P, None],
                            dict(_side_faults(6, 7, 16384), **_mesh_faults(2, 4), **_near_faults(8), **_number_faults(5, 1),
                                 **_nulls(keys=0, verts=1, faces=3, view=5, face=9, bary=10, depth=11, acc=12))),
    "nerf_raster_shade": ([P, P, P, 10, 9, P, None, P, 0, 48, 64, P, None],
                          dict(_side_faults(9, 10, 16384), **_mesh_faults(3, 4), **_nulls(face=0, bary=1, faces=2, colors=5, background=7, rgb=11),
                               **{"per_pixel 2": (8, 2), "per_pixel -1": (8, -1)})),
    "nerf_project_accumulate": ([P, P, 10, P, 9, 8, 0, 5, _views(NVIEWS), NVIEWS, 48, 64, P, P, P, 0.05, 0.01, 0.1, 0.5, 0, P, None],
                                dict(_side_faults(10, 11, 16384), **_mesh_faults(2, 4), **_near_faults(15), **_number_faults(8, NVIEWS), **_chunk(6),
                                     **_nulls(verts=0, normals=1, faces=3, views=8, images=12, depth=13, acc=14, state=20),
                                     **{k: (5, v) for k, v in TEXELS.items()},
                                     **{"n -1": (9, -1), "n 17": (9, 17), "depth_tol -1": (16, -1.0), "depth_tol nan": (16, math.nan),
                                        "cos_min 0": (17, 0.0), "cos_min 1.5": (17, 1.5), "acc_min 0": (18, 0.0), "acc_min 1.5": (18, 1.5),
                                        "mode 2": (19, 2), "state unaligned": (20, ODD)})),
    "nerf_project_finish": ([P, 9, 8, 0, 5, 1, None, P, P, None],
                            dict(_mesh_faults(None, 1), **_chunk(3), **_nulls(state=0, image=7, seen=8), **{k: (2, v) for k, v in TEXELS.items()},
                                 **{"mode 2": (5, 2), "mode -1": (5, -1), "state unaligned": (0, ODD)})),
    "nerf_mip_lod": ([P, 10, P, 9, _views(1), 0.05, 8, 1.0, P, None],
                     dict(_mesh_faults(1, 3), **_near_faults(5), **_number_faults(4, 1), **_nulls(verts=0, faces=2, view=4, lod=8),
                          **{k: (6, v) for k, v in TEXELS.items()}, **{"scale 0": (7, 0.0), "scale nan": (7, math.nan)})),
    "nerf_mip_reduce": ([P, 9, 8, P, 0, 5, None],
                        dict(_mesh_faults(None, 1), **_nulls(fine=0, coarse=3), **{k: (2, v) for k, v in TEXELS.items()},
                             **{"texels 2, the last level": (2, 2), "p0 -1": (4, -1), "count -1": (5, -1), "chunk past the end": (4, 249)})),
    "nerf_mip_sample": ([LEVELS, 9, 8, P, P, P, 1, 300, P, None],
                        dict(_mesh_faults(None, 1), **_nulls(images=0, face=3, bary=4, lod=5, rgb=8), **{k: (2, v) for k, v in TEXELS.items()},
                             **{"NULL image of level 1": (0, LEVELS_HOLE), "per_face 2": (6, 2), "n -1": (7, -1), "n 2^31": (7, 1 << 31)})),
    "nerf_texture_layout": ([9, 8, (C.c_int64 * 4)()],
                            dict(_mesh_faults(None, 0), **_nulls(out=2), **{k: (1, v) for k, v in TEXELS.items()},
                                 **{"atlas too wide": (0, 1 << 24)})),
    "nerf_texture_rows": ([P, P, 10, P, 9, 8, 0, 5, P, None],
                          dict(_mesh_faults(2, 4), **_chunk(6), **_nulls(verts=0, normals=1, faces=3, rows=8),
                               **{k: (5, v) for k, v in TEXELS.items()})),
    "nerf_texture_store": ([P, 10, P, 9, 8, 0, 5, P, None],
                           dict(_mesh_faults(1, 3), **_chunk(5), **_nulls(raw=0, faces=2, image=7), **{k: (4, v) for k, v in TEXELS.items()},
                                **{"raw unaligned": (0, ODD)})),
    "nerf_texture_uv": ([9, 8, P, None], dict(_mesh_faults(None, 0), **_nulls(uv=2), **{k: (1, v) for k, v in TEXELS.items()})),
    "nerf_texture_sample": ([P, P, P, 10, P, 9, 8, P, P, 300, P, P, None],
                            dict(_mesh_faults(3, 5), **_nulls(image=0, verts=1, normals=2, faces=4, sample_face=7, bary=8, rgb=10),
                                 **{k: (6, v) for k, v in TEXELS.items()}, **{"n -1": (9, -1), "n 2^31": (9, 1 << 31)})),
}
# the only host-only entry: its valid call launches nothing
HOST_ONLY = {"nerf_texture_layout"}
# `nothing to do`: argument lists that return NERF_OK before any launch, as {entry: {name: {position: value}}} over the valid arguments
IDLE = {
    "nerf_tsdf_integrate": {"n 0": {7: 0, 6: None, 10: None, 11: None}},
    "nerf_raster_draw": {"F 0": {3: 0, 2: None}},
    "nerf_project_accumulate": {"n 0": {9: 0, 8: None, 12: None, 20: None}, "count 0": {7: 0, 20: None, 12: None},
                                "end of the atlas": {6: 600, 7: 0}},
    "nerf_project_finish": {"count 0": {4: 0, 0: None, 7: None, 8: None}},
    "nerf_mip_lod": {"F 0": {3: 0, 2: None, 8: None}, "F 0, V 0": {3: 0, 1: 0, 0: None}},
    "nerf_mip_reduce": {"count 0": {5: 0, 0: None, 3: None}},
    "nerf_mip_sample": {"n 0": {7: 0, 0: None, 8: None}},
    "nerf_texture_rows": {"count 0": {7: 0, 8: None}},
    "nerf_texture_store": {"count 0": {6: 0, 0: None, 7: None}},
    "nerf_texture_uv": {"F 0": {0: 0, 2: None}},
    "nerf_texture_sample": {"n 0": {9: 0, 0: None, 10: None}},
}


def _calls(lib):
    """[label, rc, error text if rc != 0]"""
    rows = []

    def call(label, fn, args):
        rc = getattr(lib, fn)(*args)
        rows.append([f"{fn}: {label}", rc, lib.nerf_last_error().decode() if rc else ""])

    def with_faults(args, faults):
        out = list(args)
        for pos, v in faults:
            out[pos] = v
        return out

    for fn, (args, faults) in ENTRIES.items():
        for name, f in faults.items():
            call(name, fn, with_faults(args, [f]))
        for (na, fa), (nb, fb) in itertools.combinations(faults.items(), 2):
            if fa[0] != fb[0]:
                call(f"{na} + {nb}", fn, with_faults(args, [fa, fb]))
        for name, change in IDLE.get(fn, {}).items():
            call(f"idle, {name}", fn, with_faults(args, change.items()))
        if fn in HOST_ONLY:
            call("idle, valid", fn, args)
    return rows


def record(lib):
    return json.loads(json.dumps({"sizes": {}, "bad_calls": _calls(lib)}))


@pytest.fixture(scope="module")
def got():
    return record(N.lib())


@pytest.fixture(scope="module")
def want(got):
    with open(GOLDEN) as f:
        return expand(json.load(f), [r[0] for r in got["bad_calls"]])


def test_every_call_returns_the_recorded_code_and_text(got, want):
    g, w = got["bad_calls"], want["bad_calls"]
    assert [r[0] for r in g] == [r[0] for r in w] and len(w) > 5000
    diff = [(a, b) for a, b in zip(g, w) if a != b]
    assert not diff, diff[:5]


def test_the_recording_holds_faults_and_idle_calls_only(want):
    """No call reached a launch or the stream: a fault is NULL or SHAPE and names the entry, `nothing to do` is OK."""
    for label, rc, text in want["bad_calls"]:
        fn, what = label.split(": ", 1)
        if what.startswith("idle, "):
            assert rc == NERF_OK, label
        else:
            assert rc in (NERF_E_NULL, NERF_E_SHAPE) and text.startswith(fn + ":"), (label, rc, text)
    by = {label: (rc, text) for label, rc, text in want["bad_calls"]}
    assert by["nerf_raster_draw: view 0 number 13 nan"] == (-2, "nerf_raster_draw: non-finite camera number 13")
    assert by["nerf_project_accumulate: view 2 number 4 inf"] == (-2, "nerf_project_accumulate: view 2: non-finite camera number 4")
    assert by["nerf_tsdf_integrate: H 16777217"] == (-2, "nerf_tsdf_integrate: need 1 <= H, W <= 2^24 (got 16777217 x 64)")
    assert by["nerf_raster_resolve: W 16385 + near nan"] == (-2, "nerf_raster_resolve: need 1 <= H, W <= 16384 (got 48 x 16385)")
    assert by["nerf_mip_lod: F 2^24 + 1 + V -1"] == (-2, "nerf_mip_lod: need 0 <= V <= 2^24 (got -1)")
    assert by["nerf_mip_lod: near inf + scale 0"][1].startswith("nerf_mip_lod: near must be finite and > 0")
    assert by["nerf_mip_lod: NULL view + scale 0"][1].startswith("nerf_mip_lod: scale must be finite and > 0")
    assert by["nerf_texture_rows: V 2^24 + 1"] == (-2, "nerf_texture_rows: need 0 <= V <= 2^24 (got 16777217)")


# ------------------------------------------------------------------------------------------------ the camera, bit for bit
H, W = 48, 64
CAMS = [np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 3, 70, 70, 32, 24], np.float32),
        np.array([0.6461, -0.2449, 0.7229, 2.6, 0.0, 0.9471, 0.3209, 1.1, -0.7633, -0.2073, 0.6119, 2.2, 66.25, 66.5, 31.5, 24.25], np.float32)]


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("camera") / "camera_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "camera_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    points, checks = [[], []], {}
    for ln in out.stdout.splitlines():
        w = ln.split()
        if w[0] == "p":
            points[int(w[1])].append([int(x, 16) for x in w[2:10]] + [int(w[10]), int(w[11])])
        else:
            checks[w[1]] = [int(x) for x in w[2:]]
    return [np.array(p, np.int64) for p in points], checks


def _bits(x):
    """The bit patterns of float32 x, every NaN as one pattern (no kernel looks at a NaN's payload)."""
    x = np.ascontiguousarray(x, np.float32)
    return np.where(np.isnan(x), 0x7FC00000, x.view(np.uint32)).astype(np.int64)


@pytest.mark.parametrize("k", [0, 1])
def test_point_pixel_and_nearest_match_the_reference(printed, k):
    rows = printed[0][k]
    assert len(rows) == 900 + 32 + (8 if k == 0 else 0) + 12 + 64
    p = rows[:, 0:3].astype(np.uint32).view(np.float32)
    xc, yc, zc = CR.point(p, CAMS[k])
    u, v, _ = CR.project(p, CAMS[k])
    for col, want in zip(range(3, 8), (xc, yc, zc, u, v)):
        assert np.array_equal(_bits(rows[:, col].astype(np.uint32).view(np.float32)), _bits(want)), col
    inside, pix = CR.nearest(u, v, H, W)
    assert np.array_equal(rows[:, 8], inside.astype(np.int64))
    assert np.array_equal(rows[:, 9], pix)                                 # (0 where outside)
    # the points the list promises are there
    with np.errstate(all="ignore"):
        assert (zc < 0).sum() >= 32 and np.isnan(zc).sum() >= 3 and (~np.isfinite(u) | ~np.isfinite(v)).sum() >= 9
        assert k == 1 or ((zc == 0).sum() == 8 and (np.isnan(u) | np.isnan(v)).sum() >= 2 and np.isinf(u[zc == 0]).any())
        front = zc > 0
        for centre, coord in ((-0.5, u), (W - 0.5, u), (-0.5, v), (H - 0.5, v)):
            near_edge = front & (np.abs(coord - np.float32(centre)) < 0.5)
            assert (near_edge & inside).sum() >= 3 and (near_edge & ~inside).sum() >= 3, centre
    assert 200 < inside.sum() < len(rows) - 200


def test_argument_checks(printed):
    checks = dict(printed[1])
    assert checks.pop("views_0") == checks.pop("views_1") == checks.pop("views_16") == [NERF_OK, 1]
    for name in ("views_1_nan", "views_16_last_inf", "views_3_middle_nan"):
        assert checks.pop(name)[0] == NERF_E_SHAPE, name
    assert checks.pop("view_ok") == [NERF_OK] and checks.pop("view_null") == [NERF_E_NULL]
    assert [checks.pop(f"view_number_{q}") for q in range(16)] == [[NERF_E_SHAPE]] * 16
    assert checks.pop("near_ok") == [NERF_OK] * 2 and checks.pop("near_bad") == [NERF_E_SHAPE] * 4
    assert checks.pop("image_ok") == [NERF_OK] * 3 and checks.pop("image_bad") == [NERF_E_SHAPE] * 5
    assert not checks


if __name__ == "__main__":
    json.dump(compact(record(N.lib())), sys.stdout)
