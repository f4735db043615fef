"""Every MLP model (view / image / 2 x 64 in each of their precisions) through pack, training forward and backward at M = 65 -- two
full 32-sample tiles and a one-sample tail, padded to an 8-tile super-tile: the smallest shape with a partial tile, padding tiles
and more than one dW split -- once with "tile_pad16" 0 and once with 3.  The padding only moves the sample tiles of the fragment
stores apart, so output, gradients and d_x must be bit-equal between the two, and the stores, sized by nerf_mlp_acts_bytes /
nerf_mlp_dz_bytes, must hold everything the kernels write: a poisoned guard region behind each stays intact."""
import ctypes as C

import pytest
import torch

from nerf_meets_mlx_amd import _native as N
from tests._poison import BIG_BYTES, bits_equal, poison_, sentinel_, unwritten

pytestmark = pytest.mark.gpu
DEV = "cuda"
M = 65
GUARD = 1 << 16
# (n_layers, width, in_pos, in_dir, skip_layer, use_viewdirs, out_ch, precision)
MODELS = {"view16": (8, 256, 63, 27, 4, 1, 4, 16), "view32": (8, 256, 63, 27, 4, 1, 4, 32), "view22": (8, 256, 63, 27, 4, 1, 4, 22),
          "img16": (8, 256, 40, 0, 4, 0, 3, 16), "img32": (8, 256, 40, 0, 4, 0, 3, 32), "img22": (8, 256, 40, 0, 4, 0, 3, 22),
          "small16": (2, 64, 32, 16, -1, 1, 4, 16), "small22": (2, 64, 32, 16, -1, 1, 4, 22)}


def _guarded(nbytes):
    """A store of nbytes followed by GUARD bytes, all poisoned; (whole buffer, guard view)."""
    buf = poison_(torch.empty(nbytes + GUARD, dtype=torch.uint8, device=DEV), BIG_BYTES)
    return buf, buf[nbytes:]


def _train_pass(name, pad):
    lib = N.lib()
    arch = N.MlpArch(*MODELS[name])
    a = C.byref(arch)
    g = torch.Generator().manual_seed(5)
    params = (torch.randn(lib.nerf_mlp_param_count(a), generator=g) * 0.05).to(DEV)
    x = (torch.randn(M, arch.in_pos + arch.in_dir, generator=g) * 0.5).to(DEV)
    d_out = torch.randn(M, arch.out_ch, generator=g).to(DEV)
    before = lib.nerf_get_option(b"tile_pad16")
    N.check(lib.nerf_set_option(b"tile_pad16", pad))
    try:
        packed = torch.zeros(lib.nerf_mlp_packed_bytes(a), dtype=torch.uint8, device=DEV)
        acts, acts_guard = _guarded(lib.nerf_mlp_acts_bytes(a, M))
        dz, dz_guard = _guarded(lib.nerf_mlp_dz_bytes(a, M))
        out = sentinel_(torch.empty(M, arch.out_ch, dtype=torch.float32, device=DEV))
        grads = sentinel_(torch.empty_like(params))
        d_x = sentinel_(torch.empty(M, arch.in_pos, dtype=torch.float32, device=DEV)) if name.startswith("small") else None
        N.check(lib.nerf_mlp_pack(a, N.ptr(params), N.ptr(packed), N.stream()))
        N.check(lib.nerf_mlp_forward_train(a, N.ptr(packed), N.ptr(x), M, N.ptr(out), N.ptr(acts), N.stream()))
        if d_x is not None:
            N.check(lib.nerf_mlp_backward_inputs(a, N.ptr(packed), N.ptr(acts), N.ptr(d_out), M, N.ptr(dz), N.ptr(grads), N.ptr(d_x), N.stream()))
        else:
            N.check(lib.nerf_mlp_backward(a, N.ptr(packed), N.ptr(acts), N.ptr(d_out), M, N.ptr(dz), N.ptr(grads), N.stream()))
        torch.cuda.synchronize()
    finally:
        N.check(lib.nerf_set_option(b"tile_pad16", before))
    assert bool((acts_guard == BIG_BYTES).all()), f"{name}, tile_pad16 {pad}: a kernel wrote behind nerf_mlp_acts_bytes"
    assert bool((dz_guard == BIG_BYTES).all()), f"{name}, tile_pad16 {pad}: a kernel wrote behind nerf_mlp_dz_bytes"
    for t, what in ((out, "out"), (grads, "grads"), (d_x, "d_x")):
        if t is not None:
            assert unwritten(t) == 0 and bool(torch.isfinite(t).all()), (name, pad, what)
    assert float(out.abs().max()) > 0 and float(grads.abs().max()) > 0
    return out, grads, d_x


@pytest.mark.parametrize("name", list(MODELS))
def test_tile_padding_changes_no_result_and_the_stores_hold_every_write(name):
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    out0, grads0, dx0 = _train_pass(name, 0)
    out3, grads3, dx3 = _train_pass(name, 3)
    assert bits_equal(out0, out3), f"{name}: output differs between tile_pad16 0 and 3"
    assert bits_equal(grads0, grads3), f"{name}: gradients differ between tile_pad16 0 and 3"
    if dx0 is not None:
        assert bits_equal(dx0, dx3), f"{name}: d_x differs between tile_pad16 0 and 3"
