"""The input stage of the view model's forward kernels (csrc/mlp_input.h: sample loader, positional encodings, embedded rows,
first-layer fragments) against a recording of the parent commit, bit for bit.

tests/golden/view_inputs_parent.npz was written by `record()` below from the library of the commit BEFORE the input stage moved
into one header, on an MI355X, selected at run time and never from the code under test:
    NERF_HIP_LIB=<parent build>/libnerf_hip.so python -c "from tests.test_gpu_view_inputs import record; record()"
(tests/test_compaction_host.py documents the same procedure.)  That library was built with hipcc of HIP 7.2.26015 (AMD clang
22.0.0git, roc-7.2.0).  The precision-32 rows come from OCML's sinf / cosf / sincosf, so after a toolchain change the fixture is
recorded again from a build of that parent with the new toolchain.

Shapes (B, n): (1, 1), one sample; (11, 3), M = 33 = a full 32-sample tile + a one-sample tail = two 16-sample tiles + a tail,
with the ray index changing inside a tile (the 32-bit divide).  Depths in [2, 6]: the encodings' arguments reach the range where
the two argument reductions differ.  Model: O.init_params x 1.5 as in tests/test_gpu_pass_coverage.py.
"""
import os

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests.test_gpu_parity import _rays
from tests.test_gpu_pass_coverage import _view, options

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "view_inputs_parent.npz")
SHAPES = [(1, 1), (11, 3)]
# (precision, options) of the training cases (raw + stored encodings) and of the inference cases (raw)
TRAIN = [(16, dict(mlp_variant=v)) for v in (0, 1, 2, 3)] + [(22, {}), (32, {})]
INFER = [(16, dict(mlp_variant=v)) for v in (0, 1, 2, 3, 4, 5)] + [(22, dict(f22_tiles=t)) for t in (0, 2, 3)] + [(32, {})]


def _tag(prec, opts):
    return f"p{prec}" + "".join(f"_{k}{v}" for k, v in opts.items())


def _compute():
    """name -> array of every case (options restored by the `options` context whatever happens)."""
    from nerf_meets_mlx_amd.models.NeRF import debug_layer
    out = {}
    models = {p: _view(p)[0] for p in (16, 22, 32)}
    gx = torch.Generator().manual_seed(90)
    x = (torch.randn(33, 90, generator=gx) * 0.5).to(DEV)
    for B, n in SHAPES:
        g = torch.Generator().manual_seed(100 * B + n)
        rays = _rays(B, 10 + B).to(DEV)
        z = torch.sort(torch.rand(B, n, generator=g) * 4 + 2, -1).values.to(DEV)
        for quirk in (True, False):
            sfx = f"B{B}n{n}_q{int(quirk)}"
            for prec, opts in TRAIN:
                with options(**opts):
                    m = models[prec]
                    out[f"{_tag(prec, opts)}_train_{sfx}_raw"] = m.query(rays, z, ref_quirks=quirk, train=True).cpu().numpy()
                    out[f"{_tag(prec, opts)}_train_{sfx}_pe"] = debug_layer(m, "acts", 10).cpu().numpy()
                    out[f"{_tag(prec, opts)}_train_{sfx}_dpe"] = debug_layer(m, "acts", 11).cpu().numpy()
            for prec, opts in INFER:
                with options(**opts):
                    out[f"{_tag(prec, opts)}_infer_{sfx}_raw"] = models[prec].query(rays, z, ref_quirks=quirk).cpu().numpy()
    for prec in (16, 22, 32):                       # the embedded-row entry NeRF.forward(x)
        out[f"p{prec}_rows_train_raw"] = models[prec].forward(x, train=True).cpu().numpy()
        out[f"p{prec}_rows_infer_raw"] = models[prec].forward(x).cpu().numpy()
    torch.cuda.synchronize()
    return out


def _golden_key(k):
    """The precision-16 training variants store the same encodings: the recording keeps those of mlp_variant 1 only."""
    if k.startswith("p16_mlp_variant") and "_train_" in k and not k.endswith("_raw"):
        return "p16_mlp_variant1" + k[len("p16_mlp_variant1"):]
    return k


def record():
    assert os.environ.get("NERF_HIP_LIB"), "record() takes the PARENT commit's library through NERF_HIP_LIB"
    out = _compute()
    assert all(np.array_equal(v.view(np.uint32), out[_golden_key(k)].view(np.uint32)) for k, v in out.items())
    np.savez_compressed(GOLDEN, **{k: v for k, v in out.items() if _golden_key(k) == k})
    print(f"wrote {GOLDEN}: {os.path.getsize(GOLDEN)} bytes")


@pytest.fixture(scope="module")
def got():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return _compute()


@pytest.mark.gpu
def test_every_case_is_bit_identical_to_the_parent_recording(got):
    want = np.load(GOLDEN)
    assert sorted(want.files) == sorted({_golden_key(k) for k in got}), "the recording and the test name different cases"
    bad = [k for k, v in got.items()
           if want[_golden_key(k)].shape != v.shape or not np.array_equal(want[_golden_key(k)].view(np.uint32), v.view(np.uint32))]
    assert not bad, f"{len(bad)} of {len(got)} cases differ from the parent: {bad[:8]}"


@pytest.mark.gpu
def test_pad_columns_of_the_stored_encodings_are_zero(got):
    for k, v in got.items():
        if k.endswith("_pe"):
            assert v.shape[1] == 64 and not v[:, 63].view(np.uint32).any(), k
        if k.endswith("_dpe"):
            assert v.shape[1] == 32 and not v[:, 27:].view(np.uint32).any(), k


@pytest.mark.gpu
def test_precision_16_training_variants_store_the_same_encodings(got):
    for B, n in SHAPES:
        for q in (0, 1):
            for part in ("pe", "dpe"):
                a = got[f"p16_mlp_variant1_train_B{B}n{n}_q{q}_{part}"].view(np.uint32)
                for v in (2, 3):
                    assert np.array_equal(a, got[f"p16_mlp_variant{v}_train_B{B}n{n}_q{q}_{part}"].view(np.uint32)), (B, n, q, part, v)
