"""The host layer of the stream compactions (csrc/occupancy.hip, csrc/mesh.hip: cull, march, resumed march, marching cubes, and the
small entries beside them) against a recording of itself from before their checks, workspace layouts and march arguments were
folded onto csrc/scan.h and one MarchArgs: workspace sizes, and (return code, error text) of calls that return before any launch.
`record(lib)` below produced tests/golden/compaction_parent.json from the library of the parent commit (NERF_HIP_LIB=<that
library>, json.dump(compact(record(lib)))); the tests call it on the library under test.  No GPU: every call here returns from
argument validation or from a `nothing to do` that touches no stream."""
import ctypes as C
import itertools
import json
import math
import os

import pytest

from nerf_meets_mlx_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "compaction_parent.json")

SIZES = (0, 1, 255, 256, 257, 65, 130)
P, Q = C.c_void_p(16), C.c_void_p(48)               # non-NULL, 16-byte aligned, never dereferenced: no call below reaches a launch
ODD = C.c_void_p(8)                                 # not 16-byte aligned
LO, HI = (C.c_float * 3)(-1.0, -1.0, -1.0), (C.c_float * 3)(1.0, 1.0, 1.0)
HI_NAN, HI_LOW = (C.c_float * 3)(1.0, math.nan, 1.0), (C.c_float * 3)(1.0, 1.0, -1.0)

# the ten arguments every march entry starts with: rays, B, jitter, jitter_const, bits, log2_res, pos_scale, pos_offset,
# step_world, march_steps; and their faults as {name: (position, value)}
MARCH = [P, 613, P, 0.5, P, 7, 1.0 / 3.0, 0.5, 0.005, 64]
MARCH_FAULTS = {"log2_res 1": (5, 1), "log2_res 11": (5, 11), "B -1": (1, -1), "B 2^40": (1, 1 << 40), "march_steps 0": (9, 0),
                "march_steps 1025": (9, 1025), "step_world 0": (8, 0.0), "step_world -1": (8, -1.0), "pos_scale 0": (6, 0.0),
                "NULL rays": (0, None)}
ERT_FAULTS = {"A > B": (11, 614), "A -1": (11, -1), "B 2^31": (1, 1 << 31), "max_new 0": (13, 0), "NULL live": (10, None),
              "NULL istate": (12, None), "NULL workspace": (14, None)}

# entry -> (valid arguments: a launch, so never called as they are; faults)
ENTRIES = {
    "nerf_occ_march_count": (MARCH + [P, P, None], dict(MARCH_FAULTS, **{"NULL workspace": (10, None), "NULL offsets": (11, None)})),
    "nerf_occ_march_write": (MARCH + [P, P, P, P, None],
                             dict(MARCH_FAULTS, **{"NULL workspace": (10, None), "NULL offsets": (11, None), "NULL rows_out": (12, None),
                                                   "NULL z_out": (13, None), "B 0": (1, 0)})),
    "nerf_ert_march_count": (MARCH + [P, 333, P, 5, P, P, None], dict(MARCH_FAULTS, **ERT_FAULTS, **{"NULL totals": (15, None)})),
    "nerf_ert_march_write": (MARCH + [P, 333, P, 5, P, P, Q, P, P, None],
                             dict(MARCH_FAULTS, **ERT_FAULTS, **{"NULL offsets": (15, None), "NULL live_out": (16, None),
                                                                 "live_out == live": (16, P), "NULL rows_out": (17, None),
                                                                 "NULL z_out": (18, None)})),
    "nerf_occ_cull": ([P, P, 613, 64, P, 7, 1.0 / 3.0, 0.5, P, P, P, P, P, None, None],
                      {"log2_res 1": (5, 1), "log2_res 11": (5, 11), "B -1": (2, -1), "n -1": (3, -1), "B*n 2^50": (2, 1 << 44),
                       "raw_fill unaligned": (13, ODD), "NULL rays": (0, None), "NULL z": (1, None), "NULL bits": (4, None),
                       "NULL workspace": (8, None), "NULL idx_out": (9, None), "NULL count_out": (10, None), "NULL rays_out": (11, None),
                       "NULL z_out": (12, None)}),
    "nerf_mesh_count": ([P, 65, 0.5, P, P, None],
                        {"res 1": (1, 1), "res 513": (1, 513), "iso nan": (2, math.nan), "iso inf": (2, math.inf), "NULL vol": (0, None),
                         "NULL workspace": (3, None), "NULL totals": (4, None)}),
    "nerf_mesh_write_vertices": ([P, 65, 0.5, LO, HI, P, 1000, P, P, None, None],
                                 {"res 1": (1, 1), "res 513": (1, 513), "iso nan": (2, math.nan), "NULL lo": (3, None), "NULL hi": (4, None),
                                  "hi nan": (4, HI_NAN), "hi < lo": (4, HI_LOW), "V -1": (6, -1), "V 3 res^3 + 1": (6, 3 * 65 ** 3 + 1),
                                  "V 0": (6, 0), "NULL vol": (0, None), "NULL workspace": (5, None), "NULL verts": (7, None),
                                  "NULL normals": (8, None)}),
    "nerf_mesh_write_faces": ([P, 65, 0.5, P, 1000, P, None],
                              {"res 1": (1, 1), "res 513": (1, 513), "iso -inf": (2, -math.inf), "F -1": (4, -1),
                               "F 5 res^3 + 1": (4, 5 * 65 ** 3 + 1), "F 0": (4, 0), "NULL vol": (0, None), "NULL workspace": (3, None),
                               "NULL faces": (5, None)}),
    "nerf_occ_points": ([7, 0, 4096, 1, 2, 1.0 / 3.0, 0.5, P, P, None],
                        {"log2_res 1": (0, 1), "log2_res 11": (0, 11), "cell0 -1": (1, -1), "count -1": (2, -1), "count 2^21 + 1": (2, (1 << 21) + 1),
                         "cell0 2^21": (1, 1 << 21), "pos_scale 0": (5, 0.0), "count 0": (2, 0), "NULL rays_out": (7, None),
                         "NULL z_out": (8, None)}),
    "nerf_occ_finalize": ([P, 7, 0.01, P, None, P, None],
                          {"log2_res 1": (1, 1), "log2_res 11": (1, 11), "NULL density": (0, None), "NULL workspace": (3, None),
                           "NULL bits": (5, None)}),
    "nerf_occ_merge": ([P, P, 4096, 0.95, None], {"count -1": (2, -1), "count 0": (2, 0), "NULL density": (0, None), "NULL raw": (1, None)}),
    "nerf_occ_merge_ex": ([P, P, 4096, 0.95, 1, None],
                          {"count -1": (2, -1), "count 0": (2, 0), "activation 2": (4, 2), "activation -1": (4, -1), "NULL density": (0, None),
                           "NULL raw": (1, None)}),
    "nerf_scatter_rows": ([P, P, 300, 4, P, 1000, None],
                          {"n -1": (2, -1), "n 0": (2, 0), "channels 0": (3, 0), "n_dst -1": (5, -1), "NULL src": (0, None), "NULL idx": (1, None),
                           "NULL dst": (4, None)}),
}
# calls that would launch or touch the stream if nothing else were wrong with them: never made on their own
NO_FAULT = {"nerf_occ_merge_ex": {"NULL density, relu": [None, P, 4096, 0.95, 0, None], "NULL raw, relu": [P, None, 4096, 0.95, 0, None],
                                  "count -1, relu": [P, P, -1, 0.95, 0, None], "count 0, relu": [P, P, 0, 0.95, 0, None]}}


def _sizes(lib):
    return {"nerf_occ_march_workspace_bytes": [lib.nerf_occ_march_workspace_bytes(B) for B in SIZES + (-1, 613, 1 << 20)],
            "nerf_ert_march_workspace_bytes": [lib.nerf_ert_march_workspace_bytes(B) for B in SIZES + (-1, 613, 1 << 20)],
            "nerf_mesh_workspace_bytes": [lib.nerf_mesh_workspace_bytes(R) for R in SIZES + (-1, 2, 512, 513)],
            "nerf_occ_cull_workspace_bytes": [[lib.nerf_occ_cull_workspace_bytes(B, n) for B in SIZES + (-1,)] for n in (-1, 0, 1, 64)],
            "nerf_occ_finalize_workspace_bytes": [lib.nerf_occ_finalize_workspace_bytes(r) for r in range(0, 13)]}


def _bad_calls(lib):
    """[label, rc, error text if rc != 0]: every fault of every entry alone, then every pair of faults in two different
    arguments (which check wins is part of the behaviour)."""
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
        for name, a in NO_FAULT.get(fn, {}).items():
            call(name, fn, a)
    return rows


def record(lib):
    return json.loads(json.dumps({"sizes": _sizes(lib), "bad_calls": _bad_calls(lib)}))      # tuples -> lists, as the file reads back


def compact(rec):
    """The file form of record(): each error text once, (rc, text index) as one flat integer list, no labels."""
    msgs = [""]
    flat = []
    for _, rc, text in rec["bad_calls"]:
        if text not in msgs:
            msgs.append(text)
        flat += [rc, msgs.index(text)]
    return {"sizes": rec["sizes"], "bad_calls": flat, "messages": msgs}


def expand(data, labels):
    """Inverse of compact(); the labels are those of the list the test itself makes."""
    msgs, flat = data["messages"], data["bad_calls"]
    assert len(flat) == 2 * len(labels), "the recording holds another list of calls than _bad_calls() makes"
    return {"sizes": data["sizes"], "bad_calls": [[label, flat[2 * i], msgs[flat[2 * i + 1]]] for i, label in enumerate(labels)]}


@pytest.fixture(scope="module")
def got():
    return record(N.lib())


@pytest.fixture(scope="module")
def want(got):
    with open(GOLDEN) as f:
        return expand(json.load(f), [r[0] for r in got["bad_calls"]])


def test_workspace_sizes_match_the_recording(got, want):
    assert got["sizes"] == want["sizes"]
    s = want["sizes"]
    # the recording holds what include/nerf_hip.h states: 8 B per workgroup of 256 rays (two rows of them for the resumed march
    # and the mesh), then 4 B per ray rounded up to 8, or 4 B per lattice point
    for i, B in enumerate(SIZES):
        nblk = (B + 255) // 256
        assert s["nerf_occ_march_workspace_bytes"][i] == 8 * nblk + (4 * B + 7) // 8 * 8
        assert s["nerf_ert_march_workspace_bytes"][i] == 16 * nblk + (4 * B + 7) // 8 * 8
        assert s["nerf_mesh_workspace_bytes"][i] == (-1 if B < 2 else 16 * ((B ** 3 + 255) // 256) + 4 * B ** 3)
    assert s["nerf_occ_march_workspace_bytes"][len(SIZES)] == s["nerf_ert_march_workspace_bytes"][len(SIZES)] == -1


def test_failing_calls_return_the_recorded_code_and_text(got, want):
    g, w = got["bad_calls"], want["bad_calls"]
    assert [r[0] for r in g] == [r[0] for r in w] and len(w) > 800
    diff = [(a, b) for a, b in zip(g, w) if a != b]
    assert not diff, diff[:5]
    assert {r[1] for r in w} == {0, -1, -2}                     # OK (nothing to do), NULL, SHAPE: no call reached a launch or the stream


def test_the_recording_names_the_entry_that_was_called(want):
    for label, rc, text in want["bad_calls"]:
        fn = label.split(":")[0]
        if rc and not (fn == "nerf_occ_merge_ex" and label.endswith("relu")):      # the relu form answers as nerf_occ_merge
            assert text.startswith(fn + ":"), (label, text)
    by = {label: (rc, text) for label, rc, text in want["bad_calls"]}
    assert by["nerf_ert_march_write: log2_res 11 + A > B"] == (-2, "nerf_ert_march_write: need 2 <= log2_res <= 10")
    assert by["nerf_ert_march_write: NULL rays + A > B"] == (-1, "nerf_ert_march_write: NULL pointer")
    assert by["nerf_ert_march_write: live_out == live"] == (-2, "nerf_ert_march_write: live_out must not be live")
    assert by["nerf_occ_merge_ex: NULL raw, relu"] == (-1, "nerf_occ_merge: NULL pointer")
