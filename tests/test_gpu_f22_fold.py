"""The split-fp16 ("precision 22") inference forward with the feature layer folded into dir0 (csrc/mlp22.h, NERF_F22_FOLD).

`feature = W_F h7 + b_F` has no activation and only feeds dir0's first 256 input columns, so the packed image carries
W' = W_D[:, :256] W_F and b' = W_D[:, :256] b_F + b_D (float64 sums in index order, rounded once to float32) and the kernel runs
dir0' on [h7 | direction encoding].  The view model of tests/test_gpu_pass_coverage.py (`O.init_params x 1.5`) with b_F and b_D
overwritten by seeded N(0, 0.1) values, so that b' matters:

  1. against the float64 oracle at the sizes where the shorter weight stream can go wrong (one sample, ragged tiles, the second and
     third pass of a workgroup, a ragged last pass), both tile forms, pass queue on and off, rays + depths and embedded rows, at the
     fixture tolerance of this precision (1e-4 of the output scale, TOL[22]) -- after showing on the oracle alone that a fold
     without b_F, or with W_F transposed, moves the colours by more than 100 x that tolerance on these inputs;
  2. alpha does not see the colour branch: bit-identical alpha for two parameter sets that differ only in feature / dir0 / rgb;
  3. two parameter sets with the same W' and b' exactly (a scaled permutation as W_F) give bit-identical outputs: pins the product's
     orientation, its element order and the single rounding;
  4. one NaN in W_F or b_F makes every colour NaN and leaves alpha finite and bit-identical.
"""
import pytest
import torch

from oracle import nerf_oracle as O
from tests.test_gpu_pass_coverage import TOL, _oracle_forward, _relmax, _rows, options

pytestmark = pytest.mark.gpu
DEV = "cuda"
FWD_TOL = TOL[22]["fwd"]                       # 1e-4 of the output scale
# M = B x n samples: one sample; ragged 16-sample tiles; 129 / 193 = one more than a 128- / 192-sample pass
SMALL = {1: (1, 1), 33: (11, 3), 129: (43, 3), 193: (193, 1)}
# with 7 persistent workgroups: the second pass of a workgroup (32- and 48-sample form), the third pass + a ragged last pass
SEVEN = {7 * 128 + 1: (13, 69), 7 * 192 + 1: (5, 269), 21 * 192 + 96: (43, 96)}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"


def _spans(arch):
    """{layer: (weight offset, bias offset, out, in)} of the flat parameter buffer."""
    sp, off = {}, 0
    for name, o, i in arch.layer_shapes():
        sp[name] = (off, off + o * i, o, i)
        off += o * i + o
    return sp


def _base_flat(arch, seed=3):
    flat = O.flatten_params(arch, O.init_params(arch, seed)) * 1.5
    g = torch.Generator().manual_seed(100 + seed)
    sp = _spans(arch)
    for name in ("feature", "dir0"):
        _, b, o, _ = sp[name]
        flat[b:b + o] = torch.randn(o, generator=g) * 0.1
    return flat


def _w(flat, sp, name):
    w, _, o, i = sp[name]
    return flat[w:w + o * i].view(o, i)


def _b(flat, sp, name):
    _, b, o, _ = sp[name]
    return flat[b:b + o]


def _model(flat):
    from nerf_meets_mlx_amd.models.NeRF import NeRF
    m = NeRF(channel_input=63, channel_input_views=27, is_use_view_directions=True, device=DEV, seed=0, precision=22)
    m.load_flat(flat)
    return m


def _rays_z(B, n, seed):
    g = torch.Generator().manual_seed(seed)
    o = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=-1) * 4.0
    rays = O.pack_rays(o, -o / 4.0 + 0.25 * torch.randn(B, 3, generator=g), 2.0, 6.0)
    z = torch.sort(torch.rand(B, n, generator=g) * 4 + 2, -1).values
    return rays, z


_CASES = {}


def _case(M):
    """Rays, depths, embedded rows and the float64 oracle's outputs for M samples: computed once, shared, never modified."""
    if M not in _CASES:
        arch = O.NerfArch()
        B, n = {**SMALL, **SEVEN}[M]
        assert B * n == M
        rays, z = _rays_z(B, n, 1000 + M)
        rays, z = rays.to(DEV), z.to(DEV)
        x = _rows(rays, z).reshape(-1, 90).contiguous()
        want = _oracle_forward(arch, _base_flat(arch).to(DEV), x, False)
        _CASES[M] = (rays, z, x, want)
    return _CASES[M]


def test_the_oracle_notices_a_broken_fold():
    """On the oracle alone (CPU, float64): dropping b_F from the fold, or folding W_F transposed, moves the colours of these inputs by
    more than 100 x the tolerance of the comparison below -- so that comparison can fail for the mistakes a fold can make."""
    arch = O.NerfArch()
    sp = _spans(arch)
    flat = _base_flat(arch)
    rays, z = _rays_z(*SMALL[193], 1000 + 193)
    x = _rows(rays, z).reshape(-1, 90).double()
    with torch.no_grad():
        want = O.nerf_forward(arch, O.unflatten_params(arch, flat.double()), x)
        for what in ("b_F zeroed", "W_F transposed"):
            broken = flat.clone()
            if what == "b_F zeroed":
                _b(broken, sp, "feature").zero_()
            else:
                _w(broken, sp, "feature").copy_(_w(flat, sp, "feature").t().clone())
            got = O.nerf_forward(arch, O.unflatten_params(arch, broken.double()), x)
            moved = float((got[:, :3] - want[:, :3]).abs().max() / want.abs().max())
            print(f"oracle, {what}: colours move by {moved:.3e} of the output scale")
            assert moved > 100 * FWD_TOL, (what, moved)
            assert torch.equal(got[:, 3], want[:, 3])


@pytest.mark.parametrize("pass_queue", [1, 0])
@pytest.mark.parametrize("tiles", [2, 3])
def test_folded_forward_against_the_float64_oracle(tiles, pass_queue):
    m = _model(_base_flat(O.NerfArch()))
    worst = 0.0
    for wgs, sizes in ((0, SMALL), (7, SEVEN)):
        with options(f22_tiles=tiles, pass_queue=pass_queue, ring_workgroups=wgs):
            for M in sizes:
                rays, z, x, want = _case(M)
                for path, got in (("rays + depths", m.query(rays, z).reshape(-1, 4)), ("embedded rows", m.forward(x))):
                    assert bool(torch.isfinite(got).all()), (M, path)
                    e = _relmax(got, want)
                    print(f"f22 fold, tiles {tiles}, pass_queue {pass_queue}, ring_workgroups {wgs}, M = {M}, {path}: {e:.3e}")
                    worst = max(worst, e)
                    assert e < FWD_TOL, (tiles, pass_queue, wgs, M, path, e)
    print(f"f22 fold, tiles {tiles}, pass_queue {pass_queue}: worst {worst:.3e} of the output scale (bar {FWD_TOL:.0e})")


@pytest.mark.parametrize("tiles", [2, 3])
def test_alpha_does_not_see_the_colour_branch(tiles):
    arch = O.NerfArch()
    sp = _spans(arch)
    flat_a = _base_flat(arch)
    flat_b = flat_a.clone()
    other = _base_flat(arch, seed=5)
    for name in ("feature", "dir0", "rgb"):
        w, _, o, i = sp[name]
        flat_b[w:w + o * i + o] = other[w:w + o * i + o]
    diff = flat_a != flat_b
    assert not bool(diff[:sp["feature"][0]].any()) and not bool(diff[sp["alpha"][0]:sp["dir0"][0]].any())
    ma, mb = _model(flat_a), _model(flat_b)
    for wgs, M in ((0, 193), (7, 7 * 192 + 1)):
        rays, z, _, _ = _case(M)
        with options(f22_tiles=tiles, ring_workgroups=wgs):
            a, b = ma.query(rays, z).reshape(-1, 4), mb.query(rays, z).reshape(-1, 4)
        assert torch.equal(a[:, 3].view(torch.int32), b[:, 3].view(torch.int32)), (tiles, M)
        assert bool((a[:, :3] != b[:, :3]).any(dim=-1).all()), (tiles, M)


@pytest.mark.parametrize("tiles", [2, 3])
def test_same_folded_weights_give_the_same_bits(tiles):
    arch = O.NerfArch()
    sp = _spans(arch)
    g = torch.Generator().manual_seed(77)
    P2 = torch.zeros(256, 256, dtype=torch.float64)
    P2[torch.arange(256), torch.randperm(256, generator=g)] = 2.0
    flat_a = _base_flat(arch)
    _w(flat_a, sp, "feature").copy_(P2.float())
    bf = torch.zeros(256)
    bf[41] = 0.37
    _b(flat_a, sp, "feature").copy_(bf)
    flat_b = flat_a.clone()
    wd1 = _w(flat_a, sp, "dir0")[:, :256].double()
    _w(flat_b, sp, "feature").copy_(torch.eye(256))
    _b(flat_b, sp, "feature").zero_()
    folded = wd1 @ P2                                               # one non-zero term per sum, a power of two: exact
    assert torch.equal(folded.float().double(), folded)
    _w(flat_b, sp, "dir0")[:, :256] = folded.float()
    _b(flat_b, sp, "dir0").copy_((wd1[:, 41] * bf[41].double() + _b(flat_a, sp, "dir0").double()).float())
    ma, mb = _model(flat_a), _model(flat_b)
    rays, z, _, _ = _case(193)
    with options(f22_tiles=tiles):
        a, b = ma.query(rays, z), mb.query(rays, z)
    assert bool(torch.isfinite(a).all()) and float(a[..., :3].abs().max()) > 0
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), int((a.view(torch.int32) != b.view(torch.int32)).sum())


@pytest.mark.parametrize("where", ["W_F", "b_F"])
def test_a_nan_in_the_folded_parameters_poisons_the_colours_only(where):
    arch = O.NerfArch()
    sp = _spans(arch)
    flat = _base_flat(arch)
    rays, z, _, _ = _case(33)
    clean = _model(flat).query(rays, z)
    assert bool(torch.isfinite(clean).all())
    bad = flat.clone()
    if where == "W_F":
        _w(bad, sp, "feature")[77, 130] = float("nan")
    else:
        _b(bad, sp, "feature")[9] = float("nan")
    got = _model(bad).query(rays, z)
    assert bool(torch.isnan(got[..., :3]).all()), where
    assert torch.equal(got[..., 3].view(torch.int32), clean[..., 3].view(torch.int32)), where
