"""The host layer of the oldest units (csrc/rays.hip, sampling.hip, composite.hip, adam.hip and the closed-form encoders of
encode.hip) against a recording of itself from before their entries were folded onto shared bodies (one sample-batch body, one
compositing body, one Adam argument block) and NERF_LAUNCH: (return code, error text) of calls that return before any launch.
`record(lib)` below produced tests/golden/ray_units_parent.json from the library of the parent commit (NERF_HIP_LIB=<that library>,
json.dump(compact(record(lib)))); the test calls it on the library under test.  Which check wins when two arguments are bad, the
name nerf_adam_step_shadow answers under, and what the entries that tested `nothing to do` twice return are all part of it.
No GPU: every call here returns from argument validation or from a `nothing to do` that touches no stream."""
import ctypes as C
import itertools
import json
import os

import pytest

from nerf_meets_mlx_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ray_units_parent.json")

P, Q = C.c_void_p(16), C.c_void_p(48)               # non-NULL, 16-byte aligned, never dereferenced: no call below reaches a launch
ODD = C.c_void_p(8)                                 # not 16-byte aligned
K, C2W, FREQS = (C.c_double * 9)(), (C.c_float * 16)(), (C.c_float * 32)()      # host arguments: real memory
HW = 800 * 800

BATCH = [1000, 800, 800, 7, 5, K, C2W, 2.0, 6.0, P, P, P, P, None]
BATCH_FAULTS = {"n -1": (0, -1), "n 0": (0, 0), "H 0": (1, 0), "W 0": (2, 0), "W -1": (2, -1), "offset + n > H*W": (4, HW - 999),
                "NULL K": (5, None), "NULL c2w": (6, None), "NULL image": (9, None), "NULL rays": (10, None), "NULL target": (11, None)}
BATCH_OK = {"offset + n = H*W": (4, HW - 1000), "NULL pixel_idx": (12, None)}
ADAM = [P, P, P, P, 1000, 1e-3, 0.9, 0.999, 1e-8, 1, 1, 1.0]
ADAM_FAULTS = {"NULL params": (0, None), "NULL grads": (1, None), "NULL m": (2, None), "NULL v": (3, None), "count 0": (4, 0),
               "count -1": (4, -1), "step 0": (10, 0), "step -1": (10, -1)}
COMPOSITE_FAULTS = {"n 0": (4, 0), "n -1": (4, -1), "n 1025": (4, 1025), "B 0": (3, 0), "B -1": (3, -1), "NULL raw": (0, None),
                    "NULL z": (1, None), "NULL rays": (2, None)}
COMPOSITE_OK = {"n 1": (4, 1), "n 1024": (4, 1024)}

# entry -> (valid arguments: a launch, so never called as they are; faults as {name: (position, value)}; values that are no
# fault, at a limit or optional: a launch on their own, so only ever made together with a fault in another argument)
ENTRIES = {
    "nerf_pixel_permutation": ([P, 1000, HW, 7, 5, None],
                               {"NULL out_idx": (0, None), "n -1": (1, -1), "n 0": (1, 0), "n domain + 1": (1, HW + 1), "domain 0": (2, 0),
                                "domain -1": (2, -1), "offset + n > domain": (4, HW - 999)},
                               {"offset + n = domain": (4, HW - 1000), "seed 2^64 - 1": (3, (1 << 64) - 1)}),
    "nerf_ray_gen": ([P, 1000, 800, 800, K, C2W, 2.0, 6.0, P, P, None],
                     {"n -1": (1, -1), "n 0": (1, 0), "H 0": (2, 0), "W 0": (3, 0), "NULL K": (4, None), "NULL c2w": (5, None),
                      "NULL rays": (8, None), "NULL pixel_idx, n != H*W": (0, None)},
                     {"NULL coords": (9, None)}),
    "nerf_sample_batch": (BATCH, BATCH_FAULTS, dict(BATCH_OK, **{"unaligned image": (9, ODD), "unaligned target": (11, ODD)})),
    "nerf_sample_batch_rgba": (BATCH, dict(BATCH_FAULTS, **{"unaligned image": (9, ODD), "unaligned target": (11, ODD)}), BATCH_OK),
    "nerf_gather_rows": ([P, 1000, P, 300, 3, P, None],
                         {"n -1": (3, -1), "n 0": (3, 0), "channels 0": (4, 0), "n_src 0": (1, 0), "n_src -1": (1, -1), "NULL src": (0, None),
                          "NULL idx": (2, None), "NULL out": (5, None)},
                         {"channels 1": (4, 1), "n_src 1": (1, 1)}),
    "nerf_ndc_rays": ([P, 1000, 800, 800, 1111.0, 1.0, None], {"n 0": (1, 0), "n -1": (1, -1), "NULL rays": (0, None)}, {"H 0": (2, 0)}),
    "nerf_sample_coarse": ([P, 7, 64, 0, 1.0, P, P, None],
                           {"B -1": (1, -1), "B 0": (1, 0), "n 1": (2, 1), "n 0": (2, 0), "NULL rays": (0, None), "NULL z": (6, None),
                            "NULL t_rand, perturb 1": (5, None)},
                           {"n 2": (2, 2), "lindisp 1": (3, 1)}),
    "nerf_add_noise_z": ([P, P, 7, 64, 1.0, Q, None],
                         {"B -1": (2, -1), "B 0": (2, 0), "n 0": (3, 0), "NULL z_in": (0, None), "NULL t_rand": (1, None),
                          "NULL z_out": (5, None), "z_out == z_in": (5, P)},
                         {"n 1": (3, 1)}),
    "nerf_importance_sample": ([P, P, P, 9, 64, 128, 1e-5, P, P, P, P, None],
                               {"n 1": (4, 1), "n 257": (4, 257), "N 0": (5, 0), "N 513": (5, 513), "B 0": (3, 0),
                                "B -1": (3, -1), "NULL z": (0, None), "NULL weights": (1, None), "NULL u": (2, None)},
                               {"n 2": (4, 2), "n 256": (4, 256), "N 1": (5, 1), "N 512": (5, 512), "NULL z_new": (7, None),
                                "NULL z_merged": (8, None), "NULL cdf": (9, None), "NULL inds": (10, None)}),
    "nerf_composite_forward": ([P, P, P, 5, 64, 0.0, None, 1, P, P, P, P, P, None],
                               dict(COMPOSITE_FAULTS, **{"NULL rgb": (8, None), "noise std 1, NULL noise": (5, 1.0)}),
                               dict(COMPOSITE_OK, **{"NULL disp": (9, None), "NULL acc": (10, None), "NULL weights": (11, None),
                                                     "NULL depth": (12, None)})),
    "nerf_composite_backward": ([P, P, P, 5, 64, 0.0, None, 1, P, P, P, P, None],
                                dict(COMPOSITE_FAULTS, **{"NULL d_rgb": (8, None), "NULL d_raw": (11, None), "noise std 1, NULL noise": (5, 1.0)}),
                                dict(COMPOSITE_OK, **{"NULL d_acc": (9, None), "NULL d_depth": (10, None)})),
    "nerf_composite_mse_backward": ([P, P, P, 5, 64, 1, P, 1.0, P, P, P, None],
                                    dict(COMPOSITE_FAULTS, **{"NULL target": (6, None), "NULL d_raw": (10, None)}),
                                    dict(COMPOSITE_OK, **{"NULL loss": (8, None), "NULL rgb": (9, None)})),
    "nerf_mse_loss_grad": ([P, P, 300, 1.0, P, P, None],
                           {"NULL pred": (0, None), "NULL target": (1, None), "count 0": (2, 0), "count -1": (2, -1)},
                           {"count 1": (2, 1), "NULL loss": (4, None), "NULL d_pred": (5, None)}),
    "nerf_adam_step": (ADAM + [None], ADAM_FAULTS, {"count 1": (4, 1)}),
    "nerf_adam_step_ex": (ADAM + [0, 0, None], ADAM_FAULTS, {"count 1": (4, 1), "fixed point": (12, 1), "zero grads": (13, 1)}),
    "nerf_adam_step_shadow": (ADAM + [0, 0, P, None], ADAM_FAULTS,
                              {"count 1": (4, 1), "fixed point": (12, 1), "zero grads": (13, 1), "NULL params_half": (14, None)}),
    "nerf_encode_freq": ([P, 1000, 3, 10, 1, P, None],
                         {"M 0": (1, 0), "M -1": (1, -1), "NULL x": (0, None), "NULL out": (5, None), "D 0": (2, 0), "D 9": (2, 9),
                          "n_freqs -1": (3, -1), "n_freqs 17": (3, 17), "freq_mode 2": (4, 2), "freq_mode -1": (4, -1)},
                         {"D 1": (2, 1), "D 8": (2, 8), "n_freqs 0": (3, 0), "n_freqs 16": (3, 16), "freq_mode 0": (4, 0)}),
    "nerf_encode_sinusoidal": ([P, 1000, 3, 10, FREQS, 1, P, None],
                               {"M 0": (1, 0), "M -1": (1, -1), "NULL x": (0, None), "NULL out": (6, None), "NULL freqs": (4, None),
                                "D 0": (2, 0), "n_freqs 0": (3, 0), "n_freqs 33": (3, 33)},
                               {"D 1": (2, 1), "n_freqs 1": (3, 1), "n_freqs 32": (3, 32), "no input": (5, 0)}),
    "nerf_sh_encode": ([P, 1000, 4, P, None],
                       {"degree 5": (2, 5), "degree -1": (2, -1), "M 0": (1, 0), "M -1": (1, -1), "NULL dirs": (0, None), "NULL out": (3, None)},
                       {"degree 0": (2, 0)}),
}
# Faults that take two arguments, and faults behind a switch that the lists above leave on.  Each would launch if the fault named
# in it were mended; none is made without it.
EXTRA = {
    "nerf_ray_gen": {"NULL pixel_idx, n = H*W, NULL K": [None, HW, 800, 800, None, C2W, 2.0, 6.0, P, P, None],
                     "NULL pixel_idx, n = H*W, NULL rays": [None, HW, 800, 800, K, C2W, 2.0, 6.0, None, None, None]},
    "nerf_importance_sample": {"n 256 + N 513": [P, P, P, 9, 256, 513, 1e-5, P, P, P, P, None],
                               "n 257 + N 512": [P, P, P, 9, 257, 512, 1e-5, P, P, P, P, None],
                               "n 256 + N 512, NULL u": [P, P, None, 9, 256, 512, 1e-5, P, P, P, P, None]},
    "nerf_sample_coarse": {"NULL t_rand, perturb 0, NULL z": [P, 7, 64, 0, 0.0, None, None, None]},
    "nerf_composite_forward": {"noise std 1, noise given, NULL rgb": [P, P, P, 5, 64, 1.0, P, 1, None, P, P, P, P, None]},
    "nerf_adam_step": {"step 0, no bias correction, NULL v": [P, P, P, None, 1000, 1e-3, 0.9, 0.999, 1e-8, 0, 0, 1.0, None],
                       "step 0, no bias correction, count 0": [P, P, P, P, 0, 1e-3, 0.9, 0.999, 1e-8, 0, 0, 1.0, None]},
    "nerf_adam_step_shadow": {"step 0, no bias correction, NULL m": [P, P, None, P, 1000, 1e-3, 0.9, 0.999, 1e-8, 0, 0, 1.0, 1, 1, P, None]},
}


def _calls(lib):
    """[label, rc, error text if rc != 0]: every fault of every entry alone, every pair of faults in two different arguments
    (which check wins is part of the behaviour), every fault beside every harmless value in another argument, then EXTRA."""
    rows = []

    def call(label, fn, args):
        rc = getattr(lib, fn)(*args)
        rows.append([f"{fn}: {label}", rc, lib.nerf_last_error().decode() if rc else ""])

    def with_values(args, values):
        out = list(args)
        for pos, v in values:
            out[pos] = v
        return out

    for fn, (args, faults, harmless) in ENTRIES.items():
        for name, f in faults.items():
            call(name, fn, with_values(args, [f]))
        for (na, fa), (nb, fb) in itertools.combinations(faults.items(), 2):
            if fa[0] != fb[0]:
                call(f"{na} + {nb}", fn, with_values(args, [fa, fb]))
        for (na, fa), (nb, fb) in itertools.product(faults.items(), harmless.items()):
            if fa[0] != fb[0]:
                call(f"{na} + ({nb})", fn, with_values(args, [fa, fb]))
        for name, a in EXTRA.get(fn, {}).items():
            call(name, fn, a)
    return rows


def record(lib):
    return json.loads(json.dumps({"calls": _calls(lib)}))      # tuples -> lists, as the file reads back


def compact(rec):
    """The file form of record(): each error text once, (rc, text index) as one flat integer list, no labels."""
    msgs = [""]
    flat = []
    for _, rc, text in rec["calls"]:
        if text not in msgs:
            msgs.append(text)
        flat += [rc, msgs.index(text)]
    return {"calls": flat, "messages": msgs}


def expand(data, labels):
    """Inverse of compact(); the labels are those of the list the test itself makes."""
    msgs, flat = data["messages"], data["calls"]
    assert len(flat) == 2 * len(labels), "the recording holds another list of calls than _calls() makes"
    return {"calls": [[label, flat[2 * i], msgs[flat[2 * i + 1]]] for i, label in enumerate(labels)]}


@pytest.fixture(scope="module")
def got():
    return record(N.lib())


@pytest.fixture(scope="module")
def want(got):
    with open(GOLDEN) as f:
        return expand(json.load(f), [r[0] for r in got["calls"]])


def test_calls_return_the_recorded_code_and_text(got, want):
    g, w = got["calls"], want["calls"]
    assert [r[0] for r in g] == [r[0] for r in w] and len(w) > 1100
    diff = [(a, b) for a, b in zip(g, w) if a != b]
    assert not diff, diff[:5]
    assert {r[1] for r in w} == {0, -1, -2, -3}           # OK (nothing to do), NULL, SHAPE, UNSUPPORTED: no call reached a launch


@pytest.mark.parametrize("side", ["library", "recording"])
def test_calls_name_the_entry_that_was_called(got, want, side):
    """The same facts on the library under test and on the recording: a fixture that drifted fails as a library that did."""
    calls = (got if side == "library" else want)["calls"]
    for label, rc, text in calls:
        fn = label.split(":")[0]
        if rc:                                                                    # the shadow entry answers as nerf_adam_step_ex
            assert text.startswith(("nerf_adam_step_ex" if fn == "nerf_adam_step_shadow" else fn) + ":"), (label, text)
    by = {label: (rc, text) for label, rc, text in calls}
    assert by["nerf_adam_step_shadow: NULL m"] == (-1, "nerf_adam_step_ex: NULL pointer")
    assert by["nerf_adam_step_shadow: step 0 + (fixed point)"] == (-2, "nerf_adam_step_ex: bias correction needs step >= 1")
    assert by["nerf_adam_step: count 0 + step 0"] == (-2, "nerf_adam_step: count must be > 0")
    # the entries that tested `nothing to do` twice: the first test decides, before the NULL checks or after the shape checks
    assert by["nerf_composite_forward: B 0 + NULL raw"] == (0, "")
    assert by["nerf_composite_forward: n 0 + B 0"][0] == -2
    assert by["nerf_ray_gen: n 0 + NULL K"] == (0, "")
    assert by["nerf_ray_gen: n 0 + H 0"] == (-2, "nerf_ray_gen: bad H/W/n")
    assert by["nerf_sample_coarse: B 0 + NULL rays"] == (0, "")
    assert by["nerf_sample_coarse: B 0 + n 1"][0] == -2
    assert by["nerf_encode_freq: M 0 + freq_mode 2"] == (0, "")
    assert by["nerf_encode_sinusoidal: M -1 + n_freqs 33"] == (0, "")
    assert by["nerf_sample_batch_rgba: unaligned image"] == (-2, "nerf_sample_batch_rgba: image / target must be 16-byte aligned")
    assert by["nerf_sample_batch_rgba: NULL rays + unaligned target"] == (-1, "nerf_sample_batch_rgba: NULL pointer")
    assert by["nerf_importance_sample: n 256 + N 513"][0] == -2
    assert by["nerf_add_noise_z: z_out == z_in"][0] == -2
