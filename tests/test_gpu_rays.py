"""csrc/rays.hip on the GPU against its host mirrors (tests/_ray_ref.py), bit for bit: ray generation, the fused batch sampler, the
NDC warp and the row gather, each launched through its C ABI entry into the middle of a SENTINEL-filled buffer with guard rows.

Bars: every output word equals the mirror's (`_poison.bits_equal`).  Where the mirror's value is NaN the NaN masks are compared
instead (numpy and the device may give a computed NaN different signs); the gather's NaN rows are the constant 0x7FC00000 and are
compared as bits.  `unwritten()` of the written part is 0 and the guard rows still hold the sentinel.

Sizes: one grid trip of every kernel here is ELEMENTWISE_CAP = 2048 x 256 elements (grid_for(n, 256)); n = ELEMENTWISE_CAP + 5 runs
the second trip with a ragged tail.  What the mirrors themselves are held to: tests/test_ray_ref_host.py.
"""
import os

import numpy as np
import pytest
import torch

from nerf_meets_mlx_amd.ops.index import pixel_permutation_host
from tests import _ray_ref as R
from tests._poison import bits_equal, unwritten
from tests._render_ref import ELEMENTWISE_CAP

pytestmark = pytest.mark.gpu
DEV = "cuda"
BIG = ELEMENTWISE_CAP + 5


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _equal_or_both_nan(got, want):
    """`got` (device float32) against `want` (host float32): the NaN masks agree and every other word is bit-identical."""
    g, w = R.bits(got), np.ascontiguousarray(want).view(np.uint32)
    nan = np.isnan(want)
    return g.shape == w.shape and np.array_equal(np.isnan(got.cpu().numpy()), nan) and np.array_equal(g[~nan], w[~nan])


# ------------------------------------------------------------------------------------------------ ray generation
def _cameras(golden_dir):
    g = np.load(os.path.join(golden_dir, "ref_get_rays.npz"))
    cams = {c: tuple(int(v) for v in g[f"{c}_HW"]) + (g[f"{c}_K"], g[f"{c}_c2w"]) for c in ("small", "rect", "lego64", "lego800")}
    cams["adversarial"] = R.adversarial_camera()
    return cams, g["lego800_idx"]


def _check_ray_gen(idx_host, n, H, W, K, c2w, what):
    """Both forms (coords NULL / given) of one launch against the mirror; returns the number of 32-bit words compared."""
    p = np.arange(H * W) if idx_host is None else idx_host
    want, want_c = R.ray_gen(p, W, K, c2w, 2.0, 6.0)
    idx = None if idx_host is None else _dev(np.asarray(idx_host, np.int64))
    words = 0
    for want_coords in (False, True):
        r_full, r, c_full, c = R.ray_gen_into(idx, n, H, W, K, c2w, 2.0, 6.0, want_coords)
        assert unwritten(r) == 0 and R.guards_intact(r_full), what
        assert bits_equal(r, torch.from_numpy(want).to(DEV)), what
        words += want.size
        if want_coords:
            assert unwritten(c) == 0 and R.guards_intact(c_full), what
            assert torch.equal(c.cpu(), torch.from_numpy(want_c)), what
            words += 2 * want_c.size
    return words


def test_ray_gen_equals_the_mirror_on_every_camera(golden_dir):
    cams, lego_idx = _cameras(golden_dir)
    rng = np.random.default_rng(1)
    words = 0
    for name, (H, W, K, c2w) in cams.items():
        lists = [np.array([0]), np.array([H * W - 1]), rng.integers(0, H * W, 777), None]       # shuffled with repeats; NULL: all pixels
        if name == "lego800":
            lists.append(lego_idx)
        for p in lists:
            n = H * W if p is None else p.size
            words += _check_ray_gen(p, n, H, W, K, c2w, (name, n))
    print(f"\n[ray_gen] {words} words bit-equal to the mirror over {len(cams)} cameras")


def test_ray_gen_second_grid_trip():
    H, W, K, c2w = R.adversarial_camera()
    p = np.random.default_rng(2).integers(0, H * W, BIG)
    p[-5:] = [0, H * W - 1, W - 1, W, H * W - W]                                                # the tail of the second trip
    words = _check_ray_gen(p, BIG, H, W, K, c2w, "second trip")
    print(f"\n[ray_gen] n = {BIG}: {words} words bit-equal to the mirror")


def test_ray_gen_refusals_launch_nothing():
    H, W, K, c2w = R.adversarial_camera()
    with pytest.raises(ValueError):
        R.ray_gen_into(None, H * W - 1, H, W, K, c2w, 2.0, 6.0, False)                          # NULL index needs n == H W
    r_full, r, _, _ = R.ray_gen_into(None, 0, H, W, K, c2w, 2.0, 6.0, False)                    # n == 0: nothing happens
    assert unwritten(r_full) == r_full.numel()


# ------------------------------------------------------------------------------------------------ the fused batch and the permutation
def _check_sample_batch(n, H, W, seed, offset, K, c2w, ch, what):
    image = torch.rand(H * W, ch, generator=torch.Generator().manual_seed(3)).to(DEV)
    perm = pixel_permutation_host(n, H * W, seed, offset)
    want, _ = R.ray_gen(perm, W, K, c2w, 0.5, 9.0)
    o = R.sample_batch_into(n, H, W, seed, offset, K, c2w, 0.5, 9.0, image)
    for k, (full, inner) in o.items():
        assert unwritten(inner) == 0 and R.guards_intact(full), (what, k)
    assert torch.equal(o["idx"][1].cpu()[:, 0], torch.from_numpy(perm)), what
    assert bits_equal(o["rays"][1], torch.from_numpy(want).to(DEV)), what
    assert bits_equal(o["target"][1], image[torch.from_numpy(perm).to(DEV)]), what
    o2 = R.sample_batch_into(n, H, W, seed, offset, K, c2w, 0.5, 9.0, image, want_idx=False)    # pixel_idx NULL
    assert bits_equal(o2["rays"][1], o["rays"][1]) and bits_equal(o2["target"][1], o["target"][1]), what
    return want.size + n * ch + 2 * n


@pytest.mark.parametrize("ch", [3, 4])
def test_sample_batch_equals_the_mirror_of_the_host_permutation(ch):
    H, W, K, c2w = R.adversarial_camera()
    words = 0
    for n, seed, offset in ((H * W, 6, 0), (300, 5, 0), (100, 2 ** 63 + 11, 1000), (1, 7, H * W - 1)):
        words += _check_sample_batch(n, H, W, seed, offset, K, c2w, ch, (n, seed, offset))
    print(f"\n[sample_batch, {ch} channels] {words} words bit-equal to the mirror")


@pytest.mark.parametrize("ch", [3, 4])
def test_sample_batch_second_grid_trip(ch):
    """The smallest image that holds ELEMENTWISE_CAP + 5 pixels at the adversarial camera's (odd) width."""
    _, W, K, c2w = R.adversarial_camera()
    H = -(-BIG // W)
    assert (H - 1) * W < BIG <= H * W
    words = _check_sample_batch(BIG, H, W, 12345, H * W - BIG, K, c2w, ch, "second trip")
    print(f"\n[sample_batch, {ch} channels] n = {BIG}: {words} words bit-equal to the mirror")


def test_pixel_permutation_second_grid_trip():
    domain = 37 * 53 * 300
    full, inner = R.pixel_permutation_into(BIG, domain, 99, 17)
    assert unwritten(inner) == 0 and R.guards_intact(full)
    assert torch.equal(inner.cpu()[:, 0], torch.from_numpy(pixel_permutation_host(BIG, domain, 99, 17)))


# ------------------------------------------------------------------------------------------------ NDC
@pytest.mark.parametrize("kind", ["random", "near", "tiny_dz", "subnormal"])
def test_ndc_equals_the_mirror_and_leaves_the_other_columns(kind):
    words = 0
    for n in (1, 63, 64, 65, 1000, BIG):
        rays = R.ndc_inputs(kind, n, seed=n % 1000)
        want = R.ndc(rays.copy(), 378, 504, 400.0, 1.0)
        full, inner = R.ndc_into(rays, 378, 504, 400.0, 1.0)
        assert R.guards_intact(full), (kind, n)
        assert unwritten(inner[:, 6:]) == 5 * n, (kind, n)                                      # columns 6..10: bit-identical
        assert _equal_or_both_nan(inner[:, :6], want[:, :6]), (kind, n)
        if kind in ("random", "near", "subnormal"):
            assert np.isfinite(want[:, :6]).all() and unwritten(inner[:, :6]) == 0
        words += 11 * n
    print(f"\n[ndc {kind}] {words} words compared with the mirror")


def test_ndc_of_nothing():
    from nerf_meets_mlx_amd import _native as N
    assert N.lib().nerf_ndc_rays(None, 0, 378, 504, 400.0, 1.0, N.stream()) == 0


# ------------------------------------------------------------------------------------------------ row gather
@pytest.mark.parametrize("ch", [1, 3, 4, 7])
def test_gather_rows_equals_the_mirror_and_never_reads_outside(ch):
    """`src` is the middle of a larger buffer whose rows before and after hold the finite value 12345: a read at row -1 or n_src
    would copy that, not NaN.  n counts rows; the sizes put n * C at 1, 255 .. 257 and ELEMENTWISE_CAP + 5 elements (rounded up to
    whole rows), so the `t / C` split crosses a workgroup and a grid trip inside a row."""
    rng = np.random.default_rng(10 + ch)
    n_src = 1001
    host = rng.standard_normal((n_src + 2 * R.PAD, ch)).astype(np.float32)
    host[:R.PAD] = host[R.PAD + n_src:] = 12345.0
    buf = _dev(host)
    src = buf[R.PAD:R.PAD + n_src]
    special = np.array([0, n_src - 1, 0, n_src - 1, -1, n_src, 2 ** 40, -2 ** 40, n_src + R.PAD - 1, -R.PAD], np.int64)
    words = 0
    for elements in (1, 255, 256, 257, BIG):
        n = -(-elements // ch)
        idx = rng.integers(0, n_src, n)
        k = min(n, special.size)
        idx[n - k:] = special[:k]                                                               # the edges sit in the ragged tail
        if n > 20:
            idx[:k] = special[:k]
        want = R.gather_rows(host[R.PAD:R.PAD + n_src], idx)
        full, inner = R.gather_rows_into(src, _dev(idx))
        assert unwritten(inner) == 0 and R.guards_intact(full), (ch, n)
        assert bits_equal(inner, torch.from_numpy(want).to(DEV)), (ch, n)                       # NaN rows are 0x7FC00000 in every channel
        bad = (idx < 0) | (idx >= n_src)
        assert np.isnan(want[bad]).all() and not np.isnan(want[~bad]).any() and (n == 1 or bad.any())
        words += want.size
    print(f"\n[gather_rows C = {ch}] {words} words bit-equal to the mirror")


def test_gather_rows_refusals():
    src = torch.zeros(4, 3, device=DEV)
    idx = torch.zeros(2, dtype=torch.int64, device=DEV)
    from nerf_meets_mlx_amd import _native as N
    out = R.guarded(2, 3, DEV)[0]
    for args in ((None, 4, N.ptr(idx), 2, 3, N.ptr(out)), (N.ptr(src), 0, N.ptr(idx), 2, 3, N.ptr(out)),
                 (N.ptr(src), 4, N.ptr(idx), 2, 0, N.ptr(out))):
        with pytest.raises(ValueError):
            N.check(N.lib().nerf_gather_rows(*args, N.stream()))
    assert unwritten(out) == out.numel()
