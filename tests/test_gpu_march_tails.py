"""The march and one resumed round at sizes that end inside a wave: B = 613 rays (two full workgroups of 256, one full wave of 64,
37 lanes of the next) and a live list of A = 333 entries (256 + 64 + 13).  Every other march test uses B = 512 or 64, so none has
a partly filled wave inside a partly filled workgroup behind full ones: the lane pattern the workgroup offsets (csrc/scan.h
block_offset) must get right.  Bit for bit against tests/_march_ref.py and tests/_ert_ref.py, over poisoned buffers."""
import numpy as np
import pytest
import torch

from tests import _ert_ref as E
from tests import _march_ref as M
from tests import _occupancy_ref as O
from tests._poison import SENTINEL, bits_equal, sentinel_, unwritten
from tests.test_gpu_march import SENT64, _field, _grid, _march_poisoned, _rays

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, A, STEPS, MAX_NEW = 613, 333, 64, 5


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"


@pytest.fixture(scope="module")
def scene():
    """(grid, rays, per-ray jitter, occupancy): 30 % of the cells occupied at random."""
    from nerf_meets_mlx_amd.engine.occupancy import RES
    g = _grid(_field(), STEPS)
    gen = torch.Generator().manual_seed(21)
    occ = torch.rand(RES ** 3, generator=gen) < 0.3
    g.bits.copy_(O.pack(occ.to(DEV)))
    return g, _rays(B, 15), torch.rand(B, generator=gen).float(), occ


def test_march_of_613_rays_matches_the_reference_bit_for_bit(scene):
    from nerf_meets_mlx_amd.engine.occupancy import LOG2_RES
    g, rays, jit, occ = scene
    offs, rows, z, K = _march_poisoned(g, rays, jit.to(DEV), True)
    w_offs, w_rows, w_z, w_K = M.march(rays.cpu(), jit, occ, LOG2_RES, g.pos_scale, g.pos_offset, g.step_world, STEPS)
    cnt = w_offs[1:] - w_offs[:-1]
    assert w_K > B and int(cnt[512:].sum()) > 0 and int(cnt[576:].sum()) > 0 and bool((cnt == 0).any())     # the tail has samples
    assert K == w_K and offs.shape == (B + 1,) and torch.equal(offs.cpu(), w_offs)
    assert bits_equal(z.cpu(), w_z) and bits_equal(rows.cpu(), w_rows)
    assert unwritten(z) == 0 and unwritten(rows) == 0 and not bool((offs == SENT64).any())


def test_resumed_round_of_333_shuffled_entries_matches_the_reference(scene):
    from nerf_meets_mlx_amd.engine.occupancy import LOG2_RES
    g, rays, jit, occ = scene
    keep, zc = E.march_keep(rays.cpu(), jit, occ, LOG2_RES, g.pos_scale, g.pos_offset, g.step_world, STEPS)
    rng = np.random.default_rng(33)
    live = [int(b) for b in rng.permutation(B)[:A]]                  # shuffled: neither ascending nor dense
    terminated = {live[70], live[300]}                               # one in the first workgroup, one in the partial one
    istate = torch.zeros(B, 4, dtype=torch.int32)
    want_z, want_n, want_more = {}, {}, {}
    for b in range(B):
        kk = torch.nonzero(keep[b]).flatten().tolist()
        p = int(rng.integers(0, len(kk) + 1))                        # resume with p samples kept, anywhere in (k_{p-1}, k_p]
        lo = kk[p - 1] + 1 if p > 0 else 0
        hi = kk[p] if p < len(kk) else 2 * STEPS
        istate[b] = torch.tensor([int(rng.integers(lo, hi + 1)), p, 7, 1 if b in terminated else 0], dtype=torch.int32)
    want_state = istate.clone()
    for b in live:
        kk, p = torch.nonzero(keep[b]).flatten().tolist(), int(istate[b, 1])
        take = [] if b in terminated else kk[p:p + MAX_NEW]
        want_z[b], want_n[b] = zc[b, take], len(take)
        stopped = len(take) == MAX_NEW and p + MAX_NEW < STEPS       # at max_new, short of the cap of march_steps kept in all
        want_more[b] = stopped and take[-1] + 1 < 2 * STEPS
        if take:                                                     # (k, kept) advance; a ray that took nothing is not written
            want_state[b, 0] = take[-1] + 1 if stopped else 2 * STEPS
            want_state[b, 1] = p + len(take)
    want_K, want_A = sum(want_n[b] for b in live), sum(want_more[b] for b in live)
    assert want_K > A and 0 < want_A < A and sum(want_n[b] == 0 for b in live) > 2

    live_t = torch.tensor(live, dtype=torch.int32, device=DEV)
    jd = jit.to(DEV)
    live_out = sentinel_(torch.empty(A, dtype=torch.int32, device=DEV))
    g.march_resume(rays, jd, istate.to(DEV), live_t, A, MAX_NEW, live_out)          # grows the capacity buffers; then poison them
    for k in ("ert_rows", "ert_z"):
        sentinel_(g._cull[k])
    g._cull["ert_offsets"].fill_(SENT64)
    g._cull["ert_totals"].fill_(SENT64)
    sentinel_(live_out)
    ist = istate.to(DEV)
    offs, rows, z, K, A_next = g.march_resume(rays, jd, ist, live_t, A, MAX_NEW, live_out)
    assert (K, A_next) == (want_K, want_A)                          # the two totals
    w_offs = torch.zeros(A + 1, dtype=torch.int64)
    w_offs[1:] = torch.cumsum(torch.tensor([want_n[b] for b in live]), 0)
    assert offs.shape == (A + 1,) and torch.equal(offs.cpu(), w_offs) and int(offs[A]) == K
    assert bits_equal(z.cpu(), torch.cat([want_z[b] for b in live]))
    assert bits_equal(rows.cpu(), torch.cat([rays.cpu()[b:b + 1].expand(want_n[b], 11) for b in live]))
    assert unwritten(z) == 0 and unwritten(rows) == 0
    assert live_out[:A_next].cpu().tolist() == [b for b in live if want_more[b]]
    assert bool((live_out[A_next:] == SENTINEL).all())
    assert torch.equal(ist.cpu(), want_state)
