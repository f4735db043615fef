"""The occupancy-grid entry points of csrc/occupancy.hip over the argument space include/nerf_hip.h declares, on the GPU: every
grid size from 4^3 to 1024^3, three scene boxes (the model's, an oblique one, a mirrored one with pos_scale < 0), slices of the
grid, and every form of the row scatter.  The entries are called through the C ABI directly (OccupancyGrid fixes 128^3 and the
model's box), every output buffer poisoned first, against the references of tests/_occupancy_ref.py, tests/_march_ref.py and
tests/_ert_ref.py computed on the CPU:

  points    bit for bit against the numpy mirror; the stream's statistics (5 sigma bounds of a uniform stream) from the device's
            own points
  finalize  exact: dyadic densities make every double sum exact in any order, so thr and every word of the field are determined
  merge     slices density + cell0 between sentinels; relu bit for bit, exp within 1 ulp of the float64 exp
  cull, march, one resumed round   bit for bit, the 1024^3 grid through its 128 MiB of packed words
  scatter   float4 and scalar forms, skipped indices, the grid stride past 2048 workgroups
"""
import functools

import numpy as np
import pytest
import torch

from tests import _ert_ref as E
from tests import _march_ref as M
from tests import _occupancy_ref as O
from tests._poison import NAN_BYTES, SENTINEL, bits_equal, poison_, sentinel_, unwritten
from tests.test_gpu_march import SENT64

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOXES = {"model": (float(np.float32(1.0 / 3.0)), 0.5), "oblique": (0.37, 0.21), "mirrored": (-0.25, 0.75)}
GRIDS = [2, 3, 5, 10]                                  # points, cull, march, resume
DENSITY_GRIDS = [2, 3, 5, 9]                           # finalize, merge: the 1024^3 density alone would be 4 GiB
SEEDS = [(11, 5), (2 ** 64 - 1, 2 ** 63 + 5)]
DECAY = 0.95


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    yield
    _words.cache_clear()                               # the 1024^3 fields: 128 MiB each, on the host and on the device


def _lib():
    from nerf_meets_mlx_amd import _native as N
    return N, N.lib()


def _f32(v) -> float:
    return float(np.float32(v))


def _box(scale, offset):
    """(centre, half-width) of the box in world units, the same on every axis: the box is u = p * scale + offset in [0, 1)."""
    s, o = _f32(scale), _f32(offset)
    a, b = (0.0 - o) / s, (1.0 - o) / s
    return 0.5 * (a + b), 0.5 * abs(b - a)


def _i64(n):
    return torch.full((n,), SENT64, dtype=torch.int64, device=DEV)


def _f(*shape):
    return sentinel_(torch.empty(*shape, dtype=torch.float32, device=DEV))


def _ws(nbytes):
    return poison_(torch.empty(max(1, int(nbytes)), dtype=torch.uint8, device=DEV), NAN_BYTES)


# ------------------------------------------------------------------------------------------------ bitfields
def _random_words(nwords, seed):
    """uint32 [nwords], every bit set with probability 77 / 256 = 0.30: the binary digits of 0.01001101, last digit first, each an
    OR (digit 1: p -> (p + 1) / 2) or an AND (digit 0: p -> p / 2) with fresh random words.  No [R^3] array on the host."""
    rng = np.random.default_rng(seed)
    x = np.zeros(nwords, dtype=np.uint32)
    for digit in reversed("01001101"):
        r = rng.integers(0, 2 ** 32, nwords, dtype=np.uint32)
        x = (x | r) if digit == "1" else (x & r)
    return x


@functools.lru_cache(maxsize=None)
def _words(log2_res, kind):
    """(torch int32 words on the host, the same on the device) of a bitfield: 'random' (30 %), 'empty' or 'full'."""
    nwords = (1 << (3 * log2_res)) // 32
    w = {"random": lambda: _random_words(nwords, 100 + log2_res), "empty": lambda: np.zeros(nwords, dtype=np.uint32),
         "full": lambda: np.full(nwords, 0xFFFFFFFF, dtype=np.uint32)}[kind]()
    host = torch.from_numpy(w.view(np.int32))
    return host, host.to(DEV)


def _unpack32(words):
    """int32 [W] -> bool [32 W] on the words' device, in int32 (tests/_occupancy_ref.py unpack goes through int64)."""
    sh = torch.arange(32, dtype=torch.int32, device=words.device)
    return ((words[:, None] >> sh) & 1).reshape(-1).bool()


# ------------------------------------------------------------------------------------------------ a: points, bit for bit
POINT_SLICES = {2: [(0, 1 << 6)], 3: [(0, 1 << 9)], 5: [(0, 1 << 15)], 7: [(0, 1 << 21)],       # 2^21 rows: past 2048 x 256
                10: [(0, 1 << 20), ((1 << 30) - (1 << 20), 1 << 20)]}


def _points(log2_res, cell0, count, seed, update, scale, offset):
    N, lib = _lib()
    rays, z = _f(count, 11), _f(count)
    N.check(lib.nerf_occ_points(log2_res, cell0, count, seed, update, scale, offset, N.ptr(rays), N.ptr(z), N.stream()))
    return rays, z


@pytest.mark.parametrize("box", list(BOXES))
@pytest.mark.parametrize("log2_res", [2, 3, 5, 7, 10])
def test_points_match_the_mirror_bit_for_bit(log2_res, box):
    scale, offset = BOXES[box]
    for cell0, count in POINT_SLICES[log2_res]:
        for seed, update in SEEDS:
            want, fallback = O.points(log2_res, cell0, count, seed, update, scale, offset)
            print(f"points log2_res={log2_res} box={box} cell0={cell0} seed={seed} update={update}: "
                  f"{int(fallback.sum())} fallbacks")
            if log2_res >= 7:
                assert fallback.any()                                # the cell-centre branch is taken, and compared below
            rays, z = _points(log2_res, cell0, count, seed, update, scale, offset)
            got = rays.cpu().numpy()
            assert np.array_equal(got[:, 0:3].view(np.int32), want.view(np.int32)), (cell0, seed, update)
            assert not got[:, 3:].view(np.int32).any() and not z.cpu().numpy().view(np.int32).any()      # + 0.0 everywhere


# ------------------------------------------------------------------------------------------------ b: the stream as a jitter
def _fractions(rays, scale, offset, log2_res):
    """float64 [N, 3]: where in its cell every point of the whole grid lies, from the float32 p, pos_scale and pos_offset."""
    R = 1 << log2_res
    c = np.arange(R ** 3, dtype=np.int64)
    ci = np.stack([c & (R - 1), (c >> log2_res) & (R - 1), c >> (2 * log2_res)], 1)
    u = rays[:, 0:3].cpu().numpy().astype(np.float64) * _f32(scale) + _f32(offset)
    return u * R - ci


def _corr(a, b):
    return abs(float(np.corrcoef(a, b)[0, 1]))


@pytest.mark.parametrize("box", ["model", "mirrored"])
def test_the_stream_is_a_uniform_jitter(box):
    """Independent of the mirror: 5 sigma bounds of a uniform stream on the device's own 2^21 points of the 128^3 grid.  The mean
    of N uniforms has sigma 0.288675 / sqrt(N), the sample correlation of independent streams 1 / sqrt(N)."""
    scale, offset = BOXES[box]
    n = 1 << 21
    fr = _fractions(_points(7, 0, n, 11, 5, scale, offset)[0], scale, offset, 7)
    nxt = _fractions(_points(7, 0, n, 11, 6, scale, offset)[0], scale, offset, 7)
    assert fr.min() > -1e-3 and fr.max() < 1 + 1e-3
    mean = [abs(float(fr[:, a].mean()) - 0.5) for a in range(3)]
    axes = [_corr(fr[:, a], fr[:, b]) for a, b in ((0, 1), (0, 2), (1, 2))]
    update = [_corr(fr[:, a], nxt[:, b]) for a in range(3) for b in range(3)]
    cell = [_corr(fr[:-1, a], fr[1:, b]) for a in range(3) for b in range(3)]
    print(f"stream box={box}: mean {max(mean):.2e} (bound {5 * 0.288675 / np.sqrt(n):.2e}), axes {max(axes):.2e}, "
          f"next update {max(update):.2e}, next cell {max(cell):.2e} (bound {5 / np.sqrt(n):.2e})")
    assert max(mean) < 5 * 0.288675 / np.sqrt(n)
    assert max(axes) < 5 / np.sqrt(n) and max(update) < 5 / np.sqrt(n) and max(cell) < 5 / np.sqrt(n)


# ------------------------------------------------------------------------------------------------ c: finalize, exact
M_K = 384                                              # the strictness cases' m = 0.375, in units of 2^-10
BIG_CAP = 3.0e38


def _dyadic(k):
    return k.to(torch.float32) * (2.0 ** -10)          # k < 2^20: exact


def _random_k(n, seed):
    return torch.randint(0, 1 << 20, (n,), dtype=torch.int32, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


def _strict_k(n, seed):
    """Cells in pairs (m, m), (0, 2 m) or (2 m, 0) at random: as many 0 as 2 m, so the mean is m exactly."""
    r = torch.randint(0, 3, (n // 2,), dtype=torch.int32, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))
    a = torch.where(r == 0, M_K, torch.where(r == 1, 0, 2 * M_K)).to(torch.int32)
    return torch.stack([a, 2 * M_K - a], 1).reshape(-1)


def _finalize(density, log2_res, thr_cap, thr_out=True):
    """(thr [1] or None, words [R^3 / 32 + 2]: two sentinel words behind the field)."""
    N, lib = _lib()
    n = 1 << (3 * log2_res)
    assert density.numel() == n
    ws = _ws(lib.nerf_occ_finalize_workspace_bytes(log2_res))
    words = torch.full((n // 32 + 2,), SENTINEL, dtype=torch.int32, device=DEV)
    thr = _f(1) if thr_out else None
    N.check(lib.nerf_occ_finalize(N.ptr(density), log2_res, thr_cap, N.ptr(ws), N.ptr(thr), N.ptr(words), N.stream()))
    return thr, words


def _want_thr(k, n, thr_cap, has_inf=False) -> np.float32:
    """min(thr_cap, mean) from Python integers: total / n is exact in double (n a power of two), then one rounding to float32."""
    total = int(k.sum(dtype=torch.int64))
    mean = np.float32(np.inf) if has_inf else np.float32(total / (1024 * n))
    cap = np.float32(thr_cap)
    return mean if mean < cap else cap


def _check_finalize(density, log2_res, thr_cap, want_thr, thr_out=True):
    n = density.numel()
    thr, words = _finalize(density, log2_res, thr_cap, thr_out)
    if thr_out:
        assert int(thr.view(torch.int32)) == int(np.float32(want_thr).view(np.int32)), (float(thr), float(want_thr))
    assert bool((words[n // 32:] == SENTINEL).all())                 # nothing behind the field is written
    got = _unpack32(words[:n // 32])
    want = density > torch.tensor(float(want_thr), dtype=torch.float32, device=DEV)
    assert torch.equal(got, want), int((got != want).sum())          # every cell, none left out
    return got


@pytest.mark.parametrize("case", ["random", "strict", "cap_equal", "cap_below", "cap_above", "inf", "no_thr_out"])
@pytest.mark.parametrize("log2_res", DENSITY_GRIDS)
def test_finalize_is_exact_on_dyadic_densities(log2_res, case):
    n = 1 << (3 * log2_res)
    if case in ("random", "no_thr_out"):
        k = _random_k(n, 7 + log2_res)
        d = _dyadic(k)
        mean = _want_thr(k, n, BIG_CAP)
        got = _check_finalize(d, log2_res, BIG_CAP, mean, thr_out=case == "random")          # thr = the mean
        assert 0 < int(got.sum()) < n
        if case == "random":
            _check_finalize(d, log2_res, 100.25, np.float32(100.25))                         # thr = the cap
    elif case == "inf":
        k = _random_k(n, 17 + log2_res)
        d = _dyadic(k)
        d[n // 3] = float("inf")
        got = _check_finalize(d, log2_res, 100.25, _want_thr(k, n, 100.25, has_inf=True))
        assert bool(got[n // 3])
    else:
        k = _strict_k(n, 27 + log2_res)
        d = _dyadic(k)
        m = np.float32(M_K / 1024)
        assert int((k == 0).sum()) == int((k == 2 * M_K).sum()) > 0 and int((k == M_K).sum()) > 0
        cap = {"strict": np.float32(BIG_CAP), "cap_equal": m, "cap_below": np.nextafter(m, np.float32(-np.inf)),
               "cap_above": np.nextafter(m, np.float32(np.inf))}[case]
        want = _want_thr(k, n, cap)
        assert want == (cap if case == "cap_below" else m)
        got = _check_finalize(d, log2_res, float(cap), want)
        assert bool(got[k == 2 * M_K].all()) and not bool(got[k == 0].any())
        assert bool(got[k == M_K].all()) if case == "cap_below" else not bool(got[k == M_K].any())      # density > thr is strict


# ------------------------------------------------------------------------------------------------ d: merge on slices
MERGE_COUNTS = [1, 63, 64, 65, 257]
SPECIALS = [float("nan"), float("-inf"), float("inf"), -0.0, 88.7, 89.0]


@pytest.mark.parametrize("log2_res", DENSITY_GRIDS)
def test_merge_on_slices_between_sentinels(log2_res):
    """density + cell0 for slices at the head, the middle and the tail of the grid (a 64-cell guard on each side of it): relu bit
    for bit, exp within 1 ulp of float64 exp rounded to float32, everything outside the slice untouched.  The 4^3 grid holds 64
    cells: it has no slice of 65 or 257."""
    N, lib = _lib()
    from nerf_meets_mlx_amd.engine.occupancy import EXP, RELU
    n, G = 1 << (3 * log2_res), 64
    rng = np.random.default_rng(log2_res)
    buf = _f(n + 2 * G)
    for count in [c for c in MERGE_COUNTS if c <= n]:
        for cell0 in sorted({0, min((n - count) // 2 | 1, n - count), n - count}):
            dens = (rng.random(count) * 3.0).astype(np.float32)
            dens[:: 5] = 0.0
            raw = np.full((count, 4), np.float32(np.nan), dtype=np.float32)
            raw[:, 3] = rng.normal(0.0, 2.0, count).astype(np.float32)
            for j, v in enumerate(SPECIALS):
                raw[(j * 11 + count // 2) % count, 3] = v
            s = torch.from_numpy(raw[:, 3].copy())
            d0 = torch.from_numpy(dens)
            decayed = d0 * torch.tensor(DECAY, dtype=torch.float32)
            r64 = torch.where(torch.isnan(s), torch.zeros(count, dtype=torch.float64), torch.exp(s.double())).float()
            want_exp = torch.where(r64 > decayed, r64, decayed)
            want_relu = O.merge(d0, s, DECAY)
            raw_d = torch.from_numpy(raw).to(DEV)
            lo = G + cell0
            for how in ("merge", "ex_relu", "ex_exp"):
                buf[lo:lo + count] = d0.to(DEV)
                dp = N.ptr(buf[lo:])
                if how == "merge":
                    N.check(lib.nerf_occ_merge(dp, N.ptr(raw_d), count, DECAY, N.stream()))
                else:
                    N.check(lib.nerf_occ_merge_ex(dp, N.ptr(raw_d), count, DECAY, EXP if how == "ex_exp" else RELU, N.stream()))
                assert unwritten(buf[:lo]) == lo and unwritten(buf[lo + count:]) == n + 2 * G - lo - count, (count, cell0, how)
                got = buf[lo:lo + count].cpu()
                if how == "ex_exp":
                    ulp = (got.view(torch.int32).long() - want_exp.view(torch.int32).long()).abs()
                    assert int(ulp.max()) <= 1, (count, cell0, int(ulp.max()))
                else:
                    assert bits_equal(got, want_relu), (count, cell0, how)
                sentinel_(buf[lo:lo + count])                        # all sentinels again for the next slice


# ------------------------------------------------------------------------------------------------ e: cull
CULL_SHAPES = [(37, 29), (5, 1), (300, 64)]


def _cull_rays(B, n, seed, centre, half):
    """rays [B, 11] and sorted depths z [B, n] aimed through the box: origins within 1.3 half-widths of its centre, unit
    directions, depths up to 2.7 half-widths, so that samples fall inside and outside."""
    g = torch.Generator().manual_seed(seed)
    o = centre + (torch.rand(B, 3, generator=g) * 2 - 1) * 1.3 * half
    d = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=-1)
    rays = torch.cat([o, d, torch.zeros(B, 2), d], 1).float().contiguous()
    z = torch.sort(torch.rand(B, n, generator=g) * 2.7 * half, dim=1).values.float().contiguous()
    return rays, z


def _cull(rays, z, words, log2_res, scale, offset):
    N, lib = _lib()
    B, n = z.shape
    Mn = B * n
    idx, cnt, rk, zk, raw = _i64(Mn), _i64(1), _f(Mn, 11), _f(Mn), _f(B, n, 4)
    N.check(lib.nerf_occ_cull(N.ptr(rays), N.ptr(z), B, n, N.ptr(words), log2_res, scale, offset,
                              N.ptr(_ws(lib.nerf_occ_cull_workspace_bytes(B, n))), N.ptr(idx), N.ptr(cnt), N.ptr(rk), N.ptr(zk),
                              N.ptr(raw), N.stream()))
    return idx, int(cnt), rk, zk, raw


def _cull_case(B, n, log2_res, scale, offset, host_words):
    """The first seed whose reference is not vacuous: (rays, z, keep mask of the random field).  Needs samples outside the box,
    0 < K < B n, and at 1024^3 a kept sample in the upper half of the z cells (an index of 2^29 or more)."""
    centre, half = _box(scale, offset)
    for seed in range(200):
        rays, z = _cull_rays(B, n, 1000 * log2_res + seed, centre, half)
        c = O.cell_index(O.unit_coords(rays, z, scale, offset), log2_res)
        mask = O.occupied(host_words, c)
        K = int(mask.sum())
        high = log2_res < 10 or bool((c[mask] >> 20 >= 512).any())
        if bool((c < 0).any()) and 0 < K < B * n and high:
            return rays, z, mask
    raise AssertionError("no seed gives a case that is not vacuous")


@pytest.mark.parametrize("box", list(BOXES))
@pytest.mark.parametrize("log2_res", GRIDS)
def test_cull_at_every_grid_and_box(log2_res, box):
    scale, offset = BOXES[box]
    for B, n in CULL_SHAPES:
        rays, z, mask_random = _cull_case(B, n, log2_res, scale, offset, _words(log2_res, "random")[0])
        rd, zd = rays.to(DEV), z.to(DEV)
        for kind in ("random", "empty", "full"):
            host, dev = _words(log2_res, kind)
            mask = mask_random if kind == "random" else O.keep_mask(rays, z, host, log2_res, scale, offset)
            want = torch.nonzero(mask.reshape(-1)).reshape(-1)
            K = want.numel()
            print(f"cull log2_res={log2_res} box={box} B={B} n={n} {kind}: K={K} of {B * n}")
            assert bool((~mask).any()) and (K == 0 if kind == "empty" else K > 0)
            idx, got_K, rk, zk, raw = _cull(rd, zd, dev, log2_res, scale, offset)
            assert got_K == K and torch.equal(idx[:K].cpu(), want) and bool((idx[K:] == SENT64).all()), (B, n, kind)
            assert bits_equal(rk[:K].cpu(), rays[want // n]) and bits_equal(zk[:K].cpu(), z.reshape(-1)[want])
            assert unwritten(rk[K:]) == 11 * (B * n - K) and unwritten(zk[K:]) == B * n - K
            flat = raw.reshape(-1, 4).cpu()
            assert not bool(flat[~mask.reshape(-1)].view(torch.int32).any())                 # the zero fill
            assert unwritten(flat[mask.reshape(-1)]) == 4 * K                                # kept rows left for the scatter


# ------------------------------------------------------------------------------------------------ f: march, one resumed round
MARCH_B, MAX_NEW = 613, 5


def _march_rays(B, seed, centre, half):
    """The mix of tests/test_gpu_march.py _rays (rays from outside through the box, rays starting inside, grazing rays along a
    face, axis-parallel rays, NaN rays), its lengths scaled from a box of half-width 1.5 to this one and moved to its centre."""
    g = torch.Generator().manual_seed(seed)
    k = half / 1.5
    o = centre + (torch.rand(B, 3, generator=g) * 2 - 1) * 4.0 * k
    tgt = centre + (torch.rand(B, 3, generator=g) * 2 - 1) * 1.2 * k
    d = torch.nn.functional.normalize(tgt - o, dim=-1)
    nf = torch.tensor([[2.0 * k, 6.0 * k]]).expand(B, 2).clone()
    q = B // 8
    o[:q] = centre + (torch.rand(q, 3, generator=g) - 0.5) * 2.0 * k
    nf[:q, 0] = 0.0
    o[q:2 * q, 1] = centre + half
    d[q:2 * q, 1] = 1e-7
    d[2 * q:2 * q + 4, 2] = 0.0
    o[2 * q + 4:2 * q + 6, 0] = float("nan")
    d[2 * q + 6, 1] = float("nan")
    d = d.clone()
    return torch.cat([o, d, nf, d], 1).float().contiguous()


def _march_head(rays, jitter, words, log2_res, scale, offset, step, steps):
    N, _ = _lib()
    per_ray = torch.is_tensor(jitter)
    return (N.ptr(rays), rays.shape[0], N.ptr(jitter) if per_ray else None, 0.0 if per_ray else float(jitter), N.ptr(words), log2_res,
            scale, offset, step, steps)


def _march(rays, jitter, words, log2_res, scale, offset, step, steps):
    N, lib = _lib()
    B = rays.shape[0]
    ws, offs = _ws(lib.nerf_occ_march_workspace_bytes(B)), _i64(B + 1)
    head = _march_head(rays, jitter, words, log2_res, scale, offset, step, steps)
    N.check(lib.nerf_occ_march_count(*head, N.ptr(ws), N.ptr(offs), N.stream()))
    K = int(offs[B])
    rows, z = _f(max(1, K), 11), _f(max(1, K))
    N.check(lib.nerf_occ_march_write(*head, N.ptr(ws), N.ptr(offs), N.ptr(rows), N.ptr(z), N.stream()))
    return offs, rows[:K], z[:K], K


def _resume(rays, jitter, words, log2_res, scale, offset, step, steps):
    """One round from a fresh state, every ray live in order: (totals, offsets, rows, z, live_out, istate)."""
    N, lib = _lib()
    B = rays.shape[0]
    ws, tot, offs = _ws(lib.nerf_ert_march_workspace_bytes(B)), _i64(2), _i64(B + 1)
    istate = torch.zeros(B, 4, dtype=torch.int32, device=DEV)
    live = torch.arange(B, dtype=torch.int32, device=DEV)
    live_out = sentinel_(torch.empty(B, dtype=torch.int32, device=DEV))
    head = _march_head(rays, jitter, words, log2_res, scale, offset, step, steps) + (N.ptr(live), B)
    N.check(lib.nerf_ert_march_count(*head, N.ptr(istate), MAX_NEW, N.ptr(ws), N.ptr(tot), N.stream()))
    K, A_next = tot.tolist()
    assert 0 <= K <= MAX_NEW * B and 0 <= A_next <= B
    rows, z = _f(max(1, K), 11), _f(max(1, K))
    if K:                                                            # the product launches no write for a round without samples
        N.check(lib.nerf_ert_march_write(*head, N.ptr(istate), MAX_NEW, N.ptr(ws), N.ptr(offs), N.ptr(live_out), N.ptr(rows),
                                         N.ptr(z), N.stream()))
    return (K, A_next), offs, rows[:K], z[:K], live_out, istate


def _want_resume(rays, keep, zc, steps):
    """The round of _resume from the keep decisions of every candidate (tests/_ert_ref.py march_keep)."""
    B = rays.shape[0]
    take = keep & (torch.cumsum(keep.to(torch.int64), 1) <= MAX_NEW)
    n = take.sum(1)
    last = torch.where(take, torch.arange(2 * steps)[None, :], -1).max(1).values
    stopped = (n == MAX_NEW) & (MAX_NEW < steps)                      # at max_new, short of the cap of march_steps kept in all
    more = stopped & (last + 1 < 2 * steps)
    istate = torch.zeros(B, 4, dtype=torch.int32)
    istate[:, 0] = torch.where(n > 0, torch.where(stopped, last + 1, 2 * steps), 0).to(torch.int32)
    istate[:, 1] = n.to(torch.int32)
    offs = torch.zeros(B + 1, dtype=torch.int64)
    offs[1:] = torch.cumsum(n, 0)
    b_idx, _ = torch.nonzero(take, as_tuple=True)
    return offs, rays[b_idx], zc[take], torch.nonzero(more).flatten().to(torch.int32), istate


@pytest.mark.parametrize("box", list(BOXES))
@pytest.mark.parametrize("log2_res", GRIDS)
def test_march_and_a_resumed_round_at_every_grid_and_box(log2_res, box):
    scale, offset = BOXES[box]
    centre, half = _box(scale, offset)
    B = MARCH_B
    rays = _march_rays(B, 40 + log2_res, centre, half)
    jit_rays = torch.rand(B, generator=torch.Generator().manual_seed(41)).float()
    host, dev = _words(log2_res, "random")
    rd = rays.to(DEV)
    for steps in (1, 64):
        step = M.step_world(steps, half)
        for jitter in (jit_rays, 0.5):
            jd = jitter.to(DEV) if torch.is_tensor(jitter) else jitter
            for occ_h, occ_d in ((host, dev), (None, None)):
                tag = (steps, "rays" if torch.is_tensor(jitter) else jitter, "random" if occ_h is not None else "warmup")
                w_offs, w_rows, w_z, w_K = M.march(rays, jitter, occ_h, log2_res, scale, offset, step, steps)
                cnt = w_offs[1:] - w_offs[:-1]
                print(f"march log2_res={log2_res} box={box} {tag}: K={w_K}, {int((cnt == 0).sum())} of {B} rays without a sample")
                assert bool((cnt == 0).any()) and w_K > 0
                if steps == 64 and occ_h is not None:
                    assert w_K > B
                offs, rows, z, K = _march(rd, jd, occ_d, log2_res, scale, offset, step, steps)
                assert K == w_K and torch.equal(offs.cpu(), w_offs), tag
                assert bits_equal(z.cpu(), w_z) and bits_equal(rows.cpu(), w_rows), tag
                # one resumed round from a fresh state
                keep, zc = E.march_keep(rays, jitter, occ_h, log2_res, scale, offset, step, steps)
                r_offs, r_rows, r_z, r_live, r_state = _want_resume(rays, keep, zc, steps)
                tot, offs, rows, z, live_out, istate = _resume(rd, jd, occ_d, log2_res, scale, offset, step, steps)
                assert tot == (int(r_offs[-1]), r_live.numel()), tag
                assert tot[0] > 0 and (steps == 1 or 0 < tot[1] < B)
                assert torch.equal(offs.cpu(), r_offs) and bits_equal(z.cpu(), r_z) and bits_equal(rows.cpu(), r_rows), tag
                assert torch.equal(live_out[:tot[1]].cpu(), r_live) and bool((live_out[tot[1]:] == SENTINEL).all()), tag
                assert torch.equal(istate.cpu(), r_state), tag


# ------------------------------------------------------------------------------------------------ g: scatter
SCATTER_CASES = [(C, n, od, os_) for C in (1, 3, 4, 5) for n in (1, 255, 257) for od, os_ in ((0, 0),)] + \
                [(4, n, od, os_) for n in (1, 255, 257) for od, os_ in ((1, 0), (0, 1), (1, 1))] + [(1, 600000, 0, 0)]


@pytest.mark.parametrize("C,n,off_dst,off_src", SCATTER_CASES)
def test_scatter_rows_every_form(C, n, off_dst, off_src):
    """channels 4 with both pointers 16-byte aligned is the float4 form; an offset of one float, or any other width, the scalar
    form; 600 000 single-channel rows are past one sweep of 2048 x 256 threads.  idx is an injection into [0, n_dst) with -1,
    n_dst and 2^40 mixed in: those rows are skipped."""
    N, lib = _lib()
    rng = np.random.default_rng(1000 * C + n + 10 * off_dst + off_src)
    n_dst = n + n // 3 + 2
    idx = rng.permutation(n_dst)[:n].astype(np.int64)
    if n > 1:
        skipped = rng.permutation(n)[:min(n // 2, 3 * (1 + n // 50))]
        idx[skipped] = np.resize(np.array([-1, n_dst, 2 ** 40], dtype=np.int64), skipped.size)
    src = rng.normal(size=(n, C)).astype(np.float32)
    src_buf = torch.zeros(n * C + 4, dtype=torch.float32, device=DEV)
    dst_buf = _f(n_dst * C + 4 + 4)                                  # 4 sentinel floats behind the last row
    assert src_buf.data_ptr() % 16 == 0 and dst_buf.data_ptr() % 16 == 0
    src_d = src_buf[off_src:off_src + n * C]
    src_d.copy_(torch.from_numpy(src).reshape(-1))
    N.check(lib.nerf_scatter_rows(N.ptr(src_d), N.ptr(torch.from_numpy(idx).to(DEV)), n, C, N.ptr(dst_buf[off_dst:]), n_dst,
                                  N.stream()))
    want = np.full(dst_buf.numel(), np.int32(SENTINEL), dtype=np.int32)
    rows = want[off_dst:off_dst + n_dst * C].reshape(n_dst, C)       # a view: the numpy scatter
    ok = (idx >= 0) & (idx < n_dst)
    assert ok.any() and (n == 1 or not ok.all())
    rows[idx[ok]] = src.view(np.int32)[ok]
    assert np.array_equal(dst_buf.cpu().numpy().view(np.int32), want)


def test_scatter_of_no_rows_takes_null_pointers():
    _, lib = _lib()
    assert lib.nerf_scatter_rows(None, None, 0, 4, None, 0, None) == 0
    assert lib.nerf_scatter_rows(None, None, 0, 3, None, 10, None) == 0
