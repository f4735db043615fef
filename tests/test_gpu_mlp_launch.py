"""Every MLP kernel instantiation launched in a fresh process, where its once-per-(kernel, device) opt-in to dynamic LDS above
64 KiB has not happened yet: tests/_mlp_launch_child.py takes every model x precision of tools/ab_libs.py --models at M = 65 (two
full 32-sample tiles and one sample: a partly filled tile, fewer tiles than waves; fused queries at B = 64, n = 3) through pack,
inference forward, training forward, backward and the store reads, and through the forms that options select ("mlp_variant" 1-5,
"ring_split" 2, "f22_tiles" 2 and 3, "dw16_variant" 0, "dw22_variant" 0, level weights, fp16 shadow tables).  Child A launches
the inference forms first, child B the training forms: kernels that are opted in together meet their first launch in either order.
A launch whose opt-in was missed or came late fails (the child exits nonzero or leaves an error text) or leaves its outputs
unwritten, so both children must exit 0 with no error text and every digest of outputs, stores and gradients must be equal
between the two.  DESIGN.md 24 lists the instantiations."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_SECONDS = 120          # import and library load take most of it; the kernels are milliseconds


def _child(order):
    cmd = ["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, os.path.join(ROOT, "tests", "_mlp_launch_child.py"), order]
    out = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0, f"child {order}: exit {out.returncode}\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}"
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


def test_first_launch_of_every_mlp_kernel_in_either_order():
    a = _child("infer-first")          # (an exit code other than 0 fails here: the second child is not started)
    b = _child("train-first")
    assert a["error"] == "" and b["error"] == "", (a["error"], b["error"])
    assert len(a["digests"]) > 100 and a["digests"].keys() == b["digests"].keys()
    differing = [k for k in a["digests"] if a["digests"][k] != b["digests"][k]]
    assert not differing, f"{len(differing)} of {len(a['digests'])} digests differ between the two orders: {differing[:8]}"
