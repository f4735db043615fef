"""The occupancy references checked against each other on the host (no GPU): the numpy mirror of the jittered points
(tests/_occupancy_ref.py points) against the torch cell rule, and the packed-word lookup against the unpacked bool tensor, alone
and inside the march (tests/_march_ref.py, tests/_ert_ref.py)."""
import numpy as np
import pytest
import torch

from tests import _ert_ref as E
from tests import _march_ref as M
from tests import _occupancy_ref as O
from tests.test_march_host import OFFSET, SCALE, _rays

BOXES = [(SCALE, OFFSET), (0.37, 0.21), (-0.25, 0.75)]          # the model's, an oblique one, a mirrored power of two


def _cells(p, log2_res, scale, offset):
    """The cell of every point p [N, 3] under the torch rule (unit_coords with z = 0, cell_index)."""
    rays = torch.zeros(p.shape[0], 11)
    rays[:, 0:3] = torch.from_numpy(p)
    return O.cell_index(O.unit_coords(rays, torch.zeros(p.shape[0], 1), scale, offset)[:, 0], log2_res)


def test_mix64_is_the_splitmix64_finaliser():
    # the first outputs of splitmix64 seeded with 0: mix64 of the multiples of the golden-ratio increment
    # (Steele, Lea & Flood 2014; the published test vector of the generator)
    g = 0x9E3779B97F4A7C15
    got = [int(O.mix64((k * g) & (2 ** 64 - 1))[0]) for k in (1, 2, 3)]
    assert got == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]


@pytest.mark.parametrize("box", BOXES)
@pytest.mark.parametrize("log2_res", [2, 3, 5, 7])
def test_every_mirrored_point_maps_to_its_own_cell(log2_res, box):
    n = 1 << (3 * log2_res)
    for seed, update in ((11, 5), (2 ** 64 - 1, 2 ** 63 + 5)):
        p, fb = O.points(log2_res, 0, n, seed, update, *box)
        assert p.dtype == np.float32 and p.shape == (n, 3) and fb.shape == (n, 3)
        assert torch.equal(_cells(p, log2_res, *box), torch.arange(n))
        again, _ = O.points(log2_res, 0, n, seed, update, *box)
        assert np.array_equal(p.view(np.int32), again.view(np.int32))


@pytest.mark.parametrize("box", BOXES)
def test_slices_of_the_largest_grid_and_the_cell_centre_fallback(box):
    """At 1024^3 the first and the last 2^20 cells: every point in its cell, a slice equal to the same cells of a longer one, and
    the fallback points (which exist at this size for every box) equal to the cell centre expression."""
    s, o = np.float32(box[0]), np.float32(box[1])
    n, R = 1 << 20, 1024
    for cell0 in (0, 2 ** 30 - n):
        p, fb = O.points(10, cell0, n, 11, 5, *box)
        assert torch.equal(_cells(p, 10, *box), torch.arange(cell0, cell0 + n))
        assert fb.any() and fb.mean() < 1e-3
        c = np.arange(cell0, cell0 + n, dtype=np.int64)
        ci = np.stack([c & (R - 1), (c >> 10) & (R - 1), c >> 20], 1).astype(np.float32)
        centre = ((ci + np.float32(0.5)) * np.float32(1.0 / R) - o) / s
        assert np.array_equal(p[fb].view(np.int32), centre[fb].view(np.int32))
        assert not np.array_equal(p[~fb], centre[~fb])
        part, fb_part = O.points(10, cell0 + 777, 1000, 11, 5, *box)
        assert np.array_equal(part.view(np.int32), p[777:1777].view(np.int32)) and np.array_equal(fb_part, fb[777:1777])


def test_the_stream_depends_on_seed_update_axis_and_cell():
    p, _ = O.points(5, 0, 1 << 15, 11, 5, SCALE, OFFSET)
    for seed, update in ((12, 5), (11, 6), (11 + 2 ** 32, 5), (11, 5 + 2 ** 32)):
        q, _ = O.points(5, 0, 1 << 15, seed, update, SCALE, OFFSET)
        assert (q != p).mean() > 0.99, (seed, update)
    fr = (p.astype(np.float64) * float(np.float32(SCALE)) + OFFSET) * 32
    fr -= np.floor(fr)
    assert abs(np.corrcoef(fr[:, 0], fr[:, 1])[0, 1]) < 5 / np.sqrt(1 << 15)


@pytest.mark.parametrize("log2_res", [2, 3, 7])
def test_packed_lookup_equals_the_unpacked_bits(log2_res):
    n = 1 << (3 * log2_res)
    rng = np.random.default_rng(log2_res)
    words = rng.integers(0, 2 ** 32, n // 32, dtype=np.uint64).astype(np.uint32)
    words[0] |= np.uint32(0x80000001)                              # the sign bit of an int32 word, and bit 0
    wt = torch.from_numpy(words.view(np.int32))
    occ = O.unpack(wt)
    c = np.concatenate([rng.integers(0, n, 5000), [-1, 0, 31, 32, n - 1, -1]]).astype(np.int64)
    want = occ[torch.from_numpy(np.maximum(c, 0))] & torch.from_numpy(c >= 0)
    assert not bool(want[-1]) and not bool(want[-6]) and 0 < int(want.sum()) < c.size
    assert torch.equal(O.occupied_words(wt, torch.from_numpy(c)), want)
    assert np.array_equal(O.occupied_words(words, c), want.numpy())
    assert np.array_equal(O.occupied_words(words.view(np.int32), c.reshape(2, -1)), want.numpy().reshape(2, -1))
    assert torch.equal(O.occupied(occ, torch.from_numpy(c)), want) and torch.equal(O.occupied(words, torch.from_numpy(c)), want)
    assert torch.equal(O.pack(occ), wt)


def _gpu_mix(B, seed):
    """The ray mix of tests/test_march_host.py: rays through the box from outside, and rays that start inside it."""
    return torch.cat([_rays(B, seed), _rays(B, seed + 1, inside=True)])


def test_march_and_keep_mask_with_packed_words_equal_the_bool_tensor():
    gen = torch.Generator().manual_seed(4)
    occ = torch.rand(2 ** 21, generator=gen) < 0.3
    words = O.pack(occ)
    rays = _gpu_mix(150, 1)
    step = M.step_world(64, 1.5)
    for jitter in (0.5, torch.rand(300, generator=gen)):
        want = M.march(rays, jitter, occ, 7, SCALE, OFFSET, step, 64)
        assert want[3] > 300 and bool((want[0][1:] == want[0][:-1]).any())
        for w in (words, words.numpy().view(np.uint32)):
            got = M.march(rays, jitter, w, 7, SCALE, OFFSET, step, 64)
            assert got[3] == want[3] and all(torch.equal(a, b) for a, b in zip(got[:3], want[:3]))
            k_got, z_got = E.march_keep(rays, jitter, w, 7, SCALE, OFFSET, step, 64)
            k_want, z_want = E.march_keep(rays, jitter, occ, 7, SCALE, OFFSET, step, 64)
            assert torch.equal(k_got, k_want) and torch.equal(z_got, z_want)
    z = torch.sort(torch.rand(300, 29, generator=gen) * 4.0, dim=1).values
    want = O.keep_mask(rays, z, occ, 7, SCALE, OFFSET)
    assert 0 < int(want.sum()) < want.numel()
    assert torch.equal(O.keep_mask(rays, z, words, 7, SCALE, OFFSET), want)
    assert torch.equal(O.keep_mask(rays, z, words.numpy().view(np.uint32), 7, SCALE, OFFSET), want)
