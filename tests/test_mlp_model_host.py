"""The host layer of csrc/mlp.hip against a recording of itself from before it was rewritten around one model description
(csrc/mlp_model.h, csrc/dw_split.h): sizes, debug widths, option clamping, and (return code, error text) of calls that fail
before any launch.  `record(lib)` below produced tests/golden/mlp_model_parent.json from the library of the parent commit
(NERF_HIP_LIB=<that library>, json.dump(compact(record(lib)))); the tests call it on the library under test.  No GPU: every call
here returns from argument validation."""
import ctypes as C
import json
import math
import os
import shutil
import subprocess

import pytest

from nerf_meets_mlx_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mlp_model_parent.json")

# (n_layers, width, in_pos, in_dir, skip_layer, use_viewdirs, out_ch, precision)
ARCHS = {
    "view16": (8, 256, 63, 27, 4, 1, 4, 16), "view32": (8, 256, 63, 27, 4, 1, 4, 32), "view22": (8, 256, 63, 27, 4, 1, 4, 22),
    "img16": (8, 256, 40, 0, 4, 0, 3, 16), "img32": (8, 256, 40, 0, 4, 0, 3, 32), "img22": (8, 256, 40, 0, 4, 0, 3, 22),
    "small16": (2, 64, 32, 16, -1, 1, 4, 16), "small22": (2, 64, 32, 16, -1, 1, 4, 22),
    # not the eight supported ones
    "view0": (8, 256, 63, 27, 4, 1, 4, 0), "small32": (2, 64, 32, 16, -1, 1, 4, 32), "width128": (8, 128, 63, 27, 4, 1, 4, 16),
    "skip3": (8, 256, 63, 27, 3, 1, 4, 16), "img_out0": (8, 256, 40, 0, 4, 0, 0, 16), "img_out5": (8, 256, 40, 0, 4, 0, 5, 22),
    "img_out1_32": (8, 256, 40, 0, 4, 0, 1, 32), "img_out4_22": (8, 256, 40, 0, 4, 0, 4, 22), "prec24": (8, 256, 63, 27, 4, 1, 4, 24),
    "null": None,
}
SUPPORTED = ("view16", "view32", "view22", "img16", "img32", "img22", "small16", "small22")
MS = (-1, 0, 1, 32, 33, 65, 256, 257)
OPTION_KEYS = ("mlp_variant", "ring_split", "ring_workgroups", "tile_pad16", "dw_workgroups", "dw_unit_bias", "bwd_stage",
               "dw_job_mask", "hash_combine_max_res", "ngp_ray_major", "dw22_variant", "dw16_variant", "dw_private_tiles",
               "dw_ring_cap", "pass_queue", "dw_narrow_first", "f22_tiles", "mlp_precision", "no_such_key", None)
OPTION_VALUES = (-2 ** 31, -5, -1, 0, 1, 2, 3, 4, 5, 16, 17, 100, 2 ** 31 - 1)


def _arch(name):
    a = ARCHS[name]
    return None if a is None else C.byref(N.MlpArch(*a))


def _sizes(lib):
    out = {}
    for name in ARCHS:
        a = _arch(name)
        out[name] = {"param_count": lib.nerf_mlp_param_count(a), "packed_bytes": lib.nerf_mlp_packed_bytes(a),
                     "acts_bytes": [lib.nerf_mlp_acts_bytes(a, M) for M in MS], "dz_bytes": [lib.nerf_mlp_dz_bytes(a, M) for M in MS],
                     "debug_width": [[lib.nerf_mlp_debug_width(a, kind, layer) for layer in range(-1, 13)] for kind in (0, 1, 2)]}
    return out


def _options(lib):
    """What every key reads after every value was offered to it: [rc of set, error text of a refusal, value read back]."""
    out = {}
    for key in OPTION_KEYS:
        k = None if key is None else key.encode()
        before = lib.nerf_get_option(k)
        rows = []
        for v in OPTION_VALUES:
            rc = lib.nerf_set_option(k, v)
            rows.append([rc, lib.nerf_last_error().decode() if rc else "", lib.nerf_get_option(k)])
        if before != -2 ** 31:
            assert lib.nerf_set_option(k, before) == 0 and lib.nerf_get_option(k) == before
        out[str(key)] = {"default": before, "after": rows}
    return out


def _bad_calls(lib):
    """[label, rc, error text if rc != 0] of calls that return from validation (or from an early `nothing to do`)."""
    P = C.c_void_p(8)                                   # non-NULL, never dereferenced: every call below returns before a launch
    res = (C.c_int * 16)(*[16 << (i // 2) for i in range(16)])
    lw_ok, lw_hi, lw_neg, lw_nan = ((C.c_float * 16)(*([1.0] * 15 + [v])) for v in (0.5, 1.5, -0.1, math.nan))
    rows = []

    def call(label, fn, *args):
        rc = getattr(lib, fn)(*args)
        rows.append([f"{fn}: {label}", rc, lib.nerf_last_error().decode() if rc else ""])

    def nulls(label, fn, args, positions):
        """One NULL per pointer position, then all of them."""
        for i in positions:
            call(f"{label}, arg {i} NULL", fn, *[None if j == i else a for j, a in enumerate(args)])
        call(f"{label}, all NULL", fn, *[None if j in positions else a for j, a in enumerate(args)])

    for name in ("null", "width128", "skip3", "small32", "prec24", "img_out5"):
        a = _arch(name)
        call(f"{name}", "nerf_mlp_pack", a, P, P, None)
        call(f"{name}, NULL params", "nerf_mlp_pack", a, None, None, None)
        call(f"{name}", "nerf_mlp_forward_train", a, P, P, 65, P, P, None)
        call(f"{name}, M 0", "nerf_mlp_forward_train", a, P, P, 0, P, P, None)
        call(f"{name}", "nerf_mlp_forward", a, P, P, 65, P, None)
        call(f"{name}", "nerf_query_fused", a, P, P, P, 64, 3, 0, P, None, None)
        call(f"{name}, n 0", "nerf_query_fused", a, P, P, P, 64, 0, 0, P, None, None)
        call(f"{name}", "nerf_mlp_backward", a, P, P, P, 65, P, P, None)
        call(f"{name}, NULL packed, M 0", "nerf_mlp_backward", a, None, P, P, 0, P, P, None)
        call(f"{name}", "nerf_mlp_backward_inputs", a, P, P, P, 65, P, P, P, None)
        call(f"{name}, NULL d_x", "nerf_mlp_backward_inputs", a, P, P, P, 65, P, P, None, None)
        call(f"{name}", "nerf_ngp_query_fused", a, P, P, P, 64, 3, P, 16, 19, 2, res, 3, 1.0, 0.0, P, None, None)
        call(f"{name}, L 8", "nerf_ngp_query_fused_h", a, P, P, P, 64, 3, P, P, 8, 19, 2, res, 3, 1.0, 0.0, P, None, None)
        call(f"{name}, weight 1.5", "nerf_ngp_query_fused_lw", a, P, P, P, 64, 3, P, P, 16, 19, 2, res, lw_hi, 3, 1.0, 0.0, P, None, None)
        call(f"{name}", "nerf_mlp_debug_read", a, P, 0, 0, 65, P, None)
        call(f"{name}, layer 12, NULL store", "nerf_mlp_debug_read", a, None, 0, 12, 65, P, None)
    for name in SUPPORTED:
        a = _arch(name)
        nulls(name, "nerf_mlp_pack", [a, P, P, None], (1, 2))
        nulls(name, "nerf_mlp_forward_train", [a, P, P, 65, P, P, None], (1, 2, 4))
        for M in (0, -1):
            call(f"{name}, M {M}, all NULL", "nerf_mlp_forward_train", a, None, None, M, None, None, None)
            call(f"{name}, M {M}, all NULL", "nerf_mlp_forward", a, None, None, M, None, None)
            call(f"{name}, M {M}", "nerf_mlp_backward", a, P, P, P, M, P, P, None)
            call(f"{name}, M {M}, NULL dz", "nerf_mlp_backward", a, P, P, P, M, None, P, None)
            call(f"{name}, M {M}", "nerf_mlp_backward_inputs", a, P, P, P, M, P, P, P, None)
        nulls(name, "nerf_mlp_forward", [a, P, P, 65, P, None], (1, 2, 4))
        nulls(name, "nerf_mlp_backward", [a, P, P, P, 65, P, P, None], (1, 2, 3, 5, 6))
        call(f"{name}, NULL d_x", "nerf_mlp_backward_inputs", a, P, P, P, 65, P, P, None, None)
        call(f"{name}, NULL d_x, NULL packed, M 0", "nerf_mlp_backward_inputs", a, None, P, P, 0, P, P, None, None)
        if not name.startswith("small"):                # d_x on an 8x256 model (a supported 2x64 call would launch)
            call(f"{name}, d_x", "nerf_mlp_backward_inputs", a, P, P, P, 65, P, P, P, None)
            call(f"{name}, d_x, M 0", "nerf_mlp_backward_inputs", a, P, P, P, 0, P, P, P, None)
        nulls(f"{name}, d_x", "nerf_mlp_backward_inputs", [a, P, P, P, 65, P, P, P, None], (1, 2, 3, 5, 6))
        # the fused view-model query
        q = [a, P, P, P, 64, 3, 0, P, None, None]
        if not name.startswith("view"):
            call(f"{name}", "nerf_query_fused", *q)
        nulls(name, "nerf_query_fused", q, (1, 2, 3, 7))
        for B, n, fm, what in ((64, 0, 0, "n 0"), (0, 0, 0, "B 0, n 0"), (0, 3, 2, "B 0, freq_mode 2"), (-1, 3, 0, "B -1"),
                               (64, 3, 2, "freq_mode 2"), (64, 3, -1, "freq_mode -1"), (1 << 20, 1 << 11, 0, "B*n 2^31"),
                               (1 << 20, 1 << 11, 2, "B*n 2^31, freq_mode 2")):
            call(f"{name}, {what}", "nerf_query_fused", a, P, P, P, B, n, fm, P, None, None)
        call(f"{name}, freq_mode 2, NULL packed", "nerf_query_fused", a, None, P, P, 64, 3, 2, P, None, None)
        call(f"{name}, B*n 2^31, NULL raw", "nerf_query_fused", a, P, P, P, 1 << 20, 1 << 11, 0, None, None, None)
        # the fused hash-grid queries: (L, log2_T, F, sh_degree), B, n
        if not name.startswith("small"):
            call(f"{name}", "nerf_ngp_query_fused", a, P, P, P, 64, 3, P, 16, 19, 2, res, 3, 1.0, 0.0, P, None, None)
            call(f"{name}", "nerf_ngp_query_fused_h", a, P, P, P, 64, 3, P, P, 16, 19, 2, res, 3, 1.0, 0.0, P, None, None)
            call(f"{name}", "nerf_ngp_query_fused_lw", a, P, P, P, 64, 3, P, P, 16, 19, 2, res, lw_ok, 3, 1.0, 0.0, P, None, None)
        for (L, T, F, sh), B, n, what in (((8, 19, 2, 3), 64, 3, "L 8"), ((16, 19, 4, 3), 64, 3, "F 4"), ((16, 19, 2, 2), 64, 3, "sh 2"),
                                          ((16, 0, 2, 3), 64, 3, "log2_T 0"), ((16, 31, 2, 3), 64, 3, "log2_T 31"),
                                          ((8, 31, 2, 3), 64, 3, "L 8, log2_T 31"), ((8, 19, 2, 3), 0, 3, "L 8, B 0"),
                                          ((16, 31, 2, 3), 64, 0, "log2_T 31, n 0"), ((16, 19, 2, 3), 0, 3, "B 0"),
                                          ((16, 19, 2, 3), 64, 0, "n 0"), ((16, 19, 2, 3), -1, -1, "B -1, n -1"),
                                          ((16, 19, 2, 3), 1 << 20, 1 << 11, "B*n 2^31")):
            call(f"{name}, {what}", "nerf_ngp_query_fused", a, P, P, P, B, n, P, L, T, F, res, sh, 1.0, 0.0, P, None, None)
            call(f"{name}, {what}", "nerf_ngp_query_fused_h", a, P, P, P, B, n, P, P, L, T, F, res, sh, 1.0, 0.0, P, None, None)
            call(f"{name}, {what}, weight 1.5", "nerf_ngp_query_fused_lw", a, P, P, P, B, n, P, P, L, T, F, res, lw_hi, sh, 1.0, 0.0, P, None, None)
        nulls(name, "nerf_ngp_query_fused", [a, P, P, P, 64, 3, P, 16, 19, 2, res, 3, 1.0, 0.0, P, None, None], (1, 2, 3, 6, 10, 14))
        nulls(name, "nerf_ngp_query_fused_h", [a, P, P, P, 64, 3, P, None, 16, 19, 2, res, 3, 1.0, 0.0, P, None, None], (1, 2, 3, 6, 11, 15))
        nulls(name, "nerf_ngp_query_fused_lw", [a, P, P, P, 64, 3, P, None, 16, 19, 2, res, lw_ok, 3, 1.0, 0.0, P, None, None], (1, 2, 3, 6, 11, 16))
        for lw, what in ((lw_hi, "1.5"), (lw_neg, "-0.1"), (lw_nan, "nan")):
            call(f"{name}, weight {what}", "nerf_ngp_query_fused_lw", a, P, P, P, 64, 3, P, P, 16, 19, 2, res, lw, 3, 1.0, 0.0, P, None, None)
            call(f"{name}, weight {what}, NULL packed", "nerf_ngp_query_fused_lw", a, None, P, P, 64, 3, P, P, 16, 19, 2, res, lw, 3, 1.0, 0.0, P, None, None)
        # the test hook
        for kind, layer in ((2, 0), (-1, 0), (0, -1), (0, 12), (1, 12), (0, 2), (0, 8), (1, 8), (1, 9), (0, 10), (0, 11), (1, 11)):
            call(f"{name}, kind {kind}, layer {layer}, NULL store", "nerf_mlp_debug_read", a, None, kind, layer, 65, P, None)
            call(f"{name}, kind {kind}, layer {layer}, NULL out, M 0", "nerf_mlp_debug_read", a, P, kind, layer, 0, None, None)
            if lib.nerf_mlp_debug_width(a, kind, layer) < 0 and not name.endswith("32"):
                call(f"{name}, kind {kind}, layer {layer}", "nerf_mlp_debug_read", a, P, kind, layer, 65, P, None)
        call(f"{name}, M 0", "nerf_mlp_debug_read", a, P, 0, 0, 0, P, None)
        call(f"{name}, M -1", "nerf_mlp_debug_read", a, P, 1, 1, -1, P, None)
    return rows


def record(lib):
    out = {"options": _options(lib), "bad_calls": _bad_calls(lib)}
    before = lib.nerf_get_option(b"tile_pad16")
    try:
        for pad in (0, 3):
            assert lib.nerf_set_option(b"tile_pad16", pad) == 0
            out[f"sizes_pad{pad}"] = _sizes(lib)
    finally:
        lib.nerf_set_option(b"tile_pad16", before)
    return json.loads(json.dumps(out))          # tuples -> lists, as the file reads back


def compact(rec):
    """The file form of record(): each error text once, (rc, text index[, value]) as flat integer lists, no labels."""
    msgs = [""]

    def idx(text):
        if text not in msgs:
            msgs.append(text)
        return msgs.index(text)
    out = {k: v for k, v in rec.items() if k.startswith("sizes")}
    out["options"] = {k: [o["default"]] + [x for rc, text, val in o["after"] for x in (rc, idx(text), val)] for k, o in rec["options"].items()}
    out["bad_calls"] = [x for _, rc, text in rec["bad_calls"] for x in (rc, idx(text))]
    out["messages"] = msgs
    return out


def expand(data, labels):
    """Inverse of compact(); the labels of the calls are not in the file: they are those of the list the test itself makes."""
    msgs, flat = data["messages"], data["bad_calls"]
    assert len(flat) == 2 * len(labels), "the recording holds another list of calls than _bad_calls() makes"
    out = {k: v for k, v in data.items() if k.startswith("sizes")}
    out["options"] = {k: {"default": o[0], "after": [[o[i], msgs[o[i + 1]], o[i + 2]] for i in range(1, len(o), 3)]}
                      for k, o in data["options"].items()}
    out["bad_calls"] = [[label, flat[2 * i], msgs[flat[2 * i + 1]]] for i, label in enumerate(labels)]
    return out


@pytest.fixture(scope="module")
def got():
    return record(N.lib())


@pytest.fixture(scope="module")
def want(got):
    with open(GOLDEN) as f:
        return expand(json.load(f), [r[0] for r in got["bad_calls"]])


@pytest.mark.parametrize("pad", (0, 3))
def test_sizes_and_debug_widths_match_the_recording(got, want, pad):
    key = f"sizes_pad{pad}"
    assert set(got[key]) == set(want[key]) == set(ARCHS)
    for name in ARCHS:
        assert got[key][name] == want[key][name], (name, pad)
    for name in SUPPORTED:                      # the recording holds what it should: real sizes for the eight models ...
        s = want[key][name]
        assert s["param_count"] > 0 and s["packed_bytes"] > 0 and s["acts_bytes"][0] == -1 and min(s["acts_bytes"][2:]) > 0
    for name in set(ARCHS) - set(SUPPORTED) - {"view0", "img_out1_32", "img_out4_22"}:      # ... and -1 for what has no kernel
        s = want[key][name]
        assert s["param_count"] == -1 and s["packed_bytes"] == -1 and set(s["acts_bytes"]) == set(s["dz_bytes"]) == {-1}
    assert want[key]["view0"] == want[key]["view16"]                                        # precision 0 = the default = 16
    assert N.lib().nerf_get_option(b"tile_pad16") == 0                                      # restored


def test_padding_changes_only_the_fragment_stores(want):
    for name in SUPPORTED:
        a, b = want["sizes_pad0"][name], want["sizes_pad3"][name]
        assert a["param_count"] == b["param_count"] and a["packed_bytes"] == b["packed_bytes"] and a["debug_width"] == b["debug_width"]
        for i, M in enumerate(MS):
            tiles = (((M + 31) // 32) + 7) // 8 * 8
            extra = 0 if M < 0 or name.endswith("32") else tiles * 3 * 16      # 3 x 16 bytes per padded tile; fp32 stores: rows, no pad
            assert b["acts_bytes"][i] - a["acts_bytes"][i] == extra and b["dz_bytes"][i] - a["dz_bytes"][i] == extra, (name, M)


def test_options_clamp_and_refuse_as_recorded(got, want):
    assert got["options"] == want["options"]
    o = want["options"]
    assert [r[1] for r in o["ring_split"]["after"] if r[0]] and all(
        r[1] == "nerf_set_option: ring_split must be 1 or 2" for r in o["ring_split"]["after"] if r[0])
    assert all(r[1] == "nerf_set_option: f22_tiles must be 0 (automatic), 2 or 3" for r in o["f22_tiles"]["after"] if r[0])
    assert all(r[0] == -3 and "nerf_mlp_arch.precision" in r[1] for r in o["mlp_precision"]["after"])
    assert all(r[0] == -3 and r[1] == "nerf_set_option: unknown key 'no_such_key'" for r in o["no_such_key"]["after"])
    assert all(r[0] == -1 and r[1] == "nerf_set_option: key is NULL" for r in o["None"]["after"])


def test_failing_calls_return_the_recorded_code_and_text(got, want):
    g, w = got["bad_calls"], want["bad_calls"]
    assert [r[0] for r in g] == [r[0] for r in w] and len(w) > 1200
    diff = [(a, b) for a, b in zip(g, w) if a != b]
    assert not diff, diff[:5]
    assert {r[1] for r in w} == {0, -1, -2, -3}                 # OK (nothing to do), NULL, SHAPE, UNSUPPORTED: no call reached a launch


def test_dw_split_matches_the_recorded_table_under_sanitizers(tmp_path):
    """csrc/dw_split.h in a stand-alone program (tests/dw_split_check.cpp) built with the host compiler and
    -fsanitize=address,undefined, against tests/golden/dw_split_parent.txt."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "dw_split_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "dw_split_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "dw_split_parent.txt")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "1152 cases, 0 bad" in out.stdout
