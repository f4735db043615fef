"""Completeness of the capture table (tests/_capture.py), no GPU needed: every entry point of the C ABI that takes a stream is
classified as "captured by case N of tests/test_gpu_graph_capture.py" or "not captured here" with a reason, so a new entry point
has to be classified before the suite passes again."""
import ctypes as C
import os
import re

from nerf_meets_mlx_amd import _native as N
from tests import _capture as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_header_s_stream_entries_are_the_bound_ones():
    """The header's prototypes ending in `void* stream` are bound in _native.SIGNATURES with an int result and a pointer last, and
    no other int-returning binding ends in a pointer except nerf_comm_destroy(void* comm)."""
    entries = K.stream_entries()
    assert len(entries) > 100
    for name in entries:
        res, args = N.SIGNATURES[name]
        assert res is C.c_int and args[-1] is C.c_void_p, name
    bound = {k for k, (res, args) in N.SIGNATURES.items() if res is C.c_int and args and args[-1] is C.c_void_p}
    assert bound - set(entries) == {"nerf_comm_destroy"}


def test_every_stream_entry_is_classified_once():
    entries = set(K.stream_entries())
    both = set(K.CAPTURED) & set(K.NOT_CAPTURED)
    assert not both, sorted(both)
    missing = entries - set(K.CAPTURED) - set(K.NOT_CAPTURED)
    assert not missing, f"classify these in tests/_capture.py (CAPTURED or NOT_CAPTURED): {sorted(missing)}"
    unknown = (set(K.CAPTURED) | set(K.NOT_CAPTURED)) - entries
    assert not unknown, f"not stream-taking entry points of include/nerf_hip.h: {sorted(unknown)}"
    assert all(isinstance(c, int) and 1 <= c <= 7 for c in K.CAPTURED.values())
    assert all(isinstance(r, str) and 0 < len(r.split()) <= 12 for r in K.NOT_CAPTURED.values())


def test_captured_entries_are_called_by_the_capture_tests():
    """Every CAPTURED name is reachable from the files that hold the cases: named in the test file or its child, or in the host
    layer (nerf_meets_mlx_amd/*.py) the cases drive."""
    text = ""
    for path in ("tests/test_gpu_graph_capture.py", "tests/_capture_child.py"):
        with open(os.path.join(ROOT, path)) as f:
            text += f.read()
    pkg = os.path.join(ROOT, "nerf_meets_mlx_amd")
    for d, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith(".py") and fn != "_native.py":
                with open(os.path.join(d, fn)) as f:
                    text += f.read()
    for name in K.CAPTURED:
        assert re.search(r"\b" + name + r"\b", text), name
    # the families DESIGN.md "Graph capture" names as covered
    for name in ("nerf_ray_gen", "nerf_sample_coarse", "nerf_importance_sample", "nerf_ngp_encode_lw", "nerf_ngp_query_fused_lw",
                 "nerf_hashgrid_backward_rays_ex_lw", "nerf_mlp_pack", "nerf_query_fused", "nerf_mlp_backward", "nerf_mlp_backward_inputs",
                 "nerf_composite_forward", "nerf_composite_mse_backward", "nerf_mse_loss_grad", "nerf_adam_step", "nerf_adam_step_shadow",
                 "nerf_render_rays_fused"):
        assert name in K.CAPTURED, name
