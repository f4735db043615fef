"""The image-fitting model and the 2 x 64 hash-grid model (csrc/mlp_arch2.h, mlp_input2.h, mlp_pack.h: their index maps, kernel
arguments, fused row stage and tile map, and the one pack routine of all models) against a recording of the parent commit, bit
for bit.

tests/golden/small_models_parent.npz was written by `record()` below from the library of the commit BEFORE these were folded
into one description, on an MI355X, selected at run time and never from the code under test:
    NERF_HIP_LIB=<parent build>/libnerf_hip.so python -c "from tests.test_gpu_small_models import record; record()"
(the procedure of tests/test_gpu_view_inputs.py).  That library was built with hipcc of HIP 7.2.26015 (AMD clang 22.0.0git,
roc-7.2.0); after a toolchain change the fixture is recorded again from a build of that parent with the new toolchain.

2 x 64 model: HashNeRF(log2_hashmap_size=10) -- tiny tables, so the hashed levels collide and the fixture stays small -- with
seeded randn * 0.1 tables, bound 1.5, depths in [2, 6]; precision 16 with and without the fp16 shadow tables and precision 22;
level weights None and 16 weights with 1, fractions and 0; "ngp_ray_major" 0 and 1; training and inference; (B, n) = (1, 1), one
sample; (33, 3), M = 99: ray-major has two ray blocks, the second with one valid ray, sample-major a 3-sample tail and the ray
index changing inside a tile; (31, 2): ray-major falls back because B < 32.  Compared: raw; in training the stored input rows
(debug layers 10, 11) and, after backward on a seeded d_raw, the MLP gradient and d_x.  Plus the unfused entry mlp.forward(x) at
M = 33.  Image model: precisions 16, 22, 32 at M = 33, output and gradients.  Packed images: the eight models of
tests/test_gpu_mlp_models.py and the image model with out_ch 1 and 4, on a buffer pre-filled with one byte value.
Large results (gradients, packed images) are kept as sha256 digests, whole and per 64 KiB block, so a mismatch names the block.
"""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_mlp_models import MODELS
from tests.test_gpu_pass_coverage import _rays_z, options

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "small_models_parent.npz")
SHAPES = [(1, 1), (33, 3), (31, 2)]
FIELDS = [("p16h", 16, True), ("p16", 16, False), ("p22", 22, False)]        # (tag, precision, half_tables)
LEVEL_WEIGHTS = {"lw0": None, "lw1": (1.0, 1.0, 0.75, 0.5, 0.25, 0.0, 1.0, 0.5, 0.0, 0.125, 1.0, 1.0, 0.3, 0.0, 0.9, 1.0)}
PACKED = dict(MODELS, **{f"img{p}_oc{oc}": (8, 256, 40, 0, 4, 0, oc, p) for p in (16, 22) for oc in (1, 4)})
FILL = 0xA5
BLOCK = 1 << 16


def _digests(t):
    """sha256 of the tensor's bytes, whole and per 64 KiB block."""
    b = t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()
    return {"all": hashlib.sha256(b).hexdigest(), "blocks": [hashlib.sha256(b[i:i + BLOCK]).hexdigest() for i in range(0, len(b), BLOCK)]}


def _field(prec, half):
    from nerf_meets_mlx_amd.engine.ngp import HashNeRF
    f = HashNeRF(device=DEV, seed=0, log2_hashmap_size=10, bound=1.5, precision=prec, half_tables=half)
    f.table.load_flat(torch.randn(f.table.n_params, generator=torch.Generator().manual_seed(7)) * 0.1)
    return f


def _compute():
    """(arrays, digests): name -> array / digest record of every case (options restored by the `options` context whatever happens)."""
    from nerf_meets_mlx_amd import _native as N
    from nerf_meets_mlx_amd.models.NeRF import NeRF, debug_layer
    arrays, digests = {}, {}

    def keep(tag, mlp, raw, d_out, need_dx):
        arrays[f"{tag}_raw"] = raw.cpu().numpy()
        if d_out is None:
            return
        if need_dx:
            arrays[f"{tag}_x"] = debug_layer(mlp, "acts", 10).cpu().numpy()
            arrays[f"{tag}_dx_in"] = debug_layer(mlp, "acts", 11).cpu().numpy()
            grads, d_x = mlp.backward(d_out, need_input_grad=True)
            arrays[f"{tag}_d_x"] = d_x.cpu().numpy()
        else:
            grads = mlp.backward(d_out)
        digests[f"{tag}_grads"] = _digests(grads)

    fields = {tag: _field(prec, half) for tag, prec, half in FIELDS}
    for B, n in SHAPES:
        rays, z = _rays_z(B, n, 1000 * B + n)
        d_raw = torch.randn(B * n, 4, generator=torch.Generator().manual_seed(B + n)).to(DEV)
        for tag, f in fields.items():
            for lw_tag, lw in LEVEL_WEIGHTS.items():
                f.level_weights = lw
                for rm in (0, 1):
                    with options(ngp_ray_major=rm):
                        name = f"{tag}_{lw_tag}_rm{rm}_B{B}n{n}"
                        keep(name + "_infer", f.mlp, f.query(rays, z).reshape(-1, 4), None, True)
                        keep(name + "_train", f.mlp, f.query(rays, z, train=True).reshape(-1, 4), d_raw, True)
    g = torch.Generator().manual_seed(48)
    x = (torch.randn(33, 48, generator=g) * 0.5).to(DEV)
    d_raw = torch.randn(33, 4, generator=g).to(DEV)
    for tag in ("p16", "p22"):                       # the embedded-row entry NeRF.forward(x)
        mlp = fields[tag].mlp
        keep(f"{tag}_rows_infer", mlp, mlp.forward(x), None, True)
        keep(f"{tag}_rows_train", mlp, mlp.forward(x, train=True), d_raw, True)
    g = torch.Generator().manual_seed(40)
    x = (torch.randn(33, 40, generator=g) * 0.5).to(DEV)
    d_out = torch.randn(33, 3, generator=g).to(DEV)
    for prec in (16, 22, 32):
        m = NeRF(channel_input=40, channel_input_views=0, channel_output=3, is_use_view_directions=False, device=DEV, seed=2, precision=prec)
        keep(f"img{prec}_infer", m, m.forward(x), None, False)
        keep(f"img{prec}_train", m, m.forward(x, train=True), d_out, False)
    lib = N.lib()
    for name, spec in PACKED.items():
        a = C.byref(N.MlpArch(*spec))
        params = (torch.randn(lib.nerf_mlp_param_count(a), generator=torch.Generator().manual_seed(5)) * 0.05).to(DEV)
        packed = torch.full((lib.nerf_mlp_packed_bytes(a),), FILL, dtype=torch.uint8, device=DEV)
        N.check(lib.nerf_mlp_pack(a, N.ptr(params), N.ptr(packed), N.stream()))
        digests[f"packed_{name}"] = _digests(packed)
    torch.cuda.synchronize()
    return arrays, digests


def _golden_key(k):
    """Training keeps activations, and ray-major tiles exist only without them: the recording keeps the "ngp_ray_major" 0 cases."""
    return k.replace("_rm1_", "_rm0_") if "_train" in k else k


def record():
    assert os.environ.get("NERF_HIP_LIB"), "record() takes the PARENT commit's library through NERF_HIP_LIB"
    arrays, digests = _compute()
    assert all(np.array_equal(v.view(np.uint32), arrays[_golden_key(k)].view(np.uint32)) for k, v in arrays.items())
    assert all(v == digests[_golden_key(k)] for k, v in digests.items())
    blob = json.dumps({k: v for k, v in digests.items() if _golden_key(k) == k}, sort_keys=True).encode()
    np.savez_compressed(GOLDEN, digests=np.frombuffer(blob, dtype=np.uint8), **{k: v for k, v in arrays.items() if _golden_key(k) == k})
    print(f"wrote {GOLDEN}: {os.path.getsize(GOLDEN)} bytes, {len(arrays)} arrays, {len(digests)} digests")


@pytest.fixture(scope="module")
def got():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return _compute()


@pytest.fixture(scope="module")
def want():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files if k != "digests"}, json.loads(z["digests"].tobytes().decode())


@pytest.mark.gpu
def test_the_recording_and_the_test_name_the_same_cases(got, want):
    assert sorted(want[0]) == sorted({_golden_key(k) for k in got[0]}), "the recording and the test name different arrays"
    assert sorted(want[1]) == sorted({_golden_key(k) for k in got[1]}), "the recording and the test name different digests"


@pytest.mark.gpu
def test_every_output_is_bit_identical_to_the_parent_recording(got, want):
    bad = [k for k, v in got[0].items()
           if want[0][_golden_key(k)].shape != v.shape or not np.array_equal(want[0][_golden_key(k)].view(np.uint32), v.view(np.uint32))]
    assert not bad, f"{len(bad)} of {len(got[0])} arrays differ from the parent: {bad[:8]}"


@pytest.mark.gpu
def test_every_gradient_and_packed_image_is_bit_identical_to_the_parent_recording(got, want):
    bad = []
    for k, v in got[1].items():
        w = want[1][_golden_key(k)]
        if v != w:
            blocks = [i for i, (a, b) in enumerate(zip(v["blocks"], w["blocks"])) if a != b]
            bad.append((k, f"{len(v['blocks'])} blocks against {len(w['blocks'])}" if len(v["blocks"]) != len(w["blocks"]) else f"64 KiB blocks {blocks[:8]}"))
    assert not bad, f"{len(bad)} of {len(got[1])} digests differ from the parent: {bad[:8]}"
