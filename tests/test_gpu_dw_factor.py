"""The factored weight gradients of the 8 x 256 view model at precision 22 (nerf_set_option("dw_factor", 1); csrc/mlp_model.h:
VIEW_JOBS_FACTORED, csrc/mlp_dwf.hip).  feature = W_F h7 + b_F has no activation (models/NeRF.py:231), so with
    G = dZ_D^T H7  [128, 256],   db_D = column sums of dZ_D
the gradients of the feature layer and of the feature columns of dir0 are, exactly,
    dW_F = W_D[:, :256]^T G,   db_F = W_D[:, :256]^T db_D,   dW_D[:, :256] = G W_F^T + db_D b_F^T
and ONE dW job (d alpha | dZ_D against H7) + a post step replace the three jobs feature, alpha and dir0 | feature.

Reference of the first test: the three formulas in float64 on the host, on the operands the kernels themselves stored (H7, dZ_D,
d alpha through nerf_mlp_debug_read) and on the weights the chain and the forward multiply with (bf16(w) + bf16(w - bf16(w))).
Bounds: the project's precision-22 gradient bounds, TOL_SMALL[22] of tests/test_gpu_pass_coverage.py (rel-L2 <= 1e-4,
rel-max <= 1e-3)."""
import ctypes as C

import pytest
import torch

from tests.test_gpu_pass_coverage import TOL_SMALL, _rays_z, _rel_l2, _relmax, _view, options

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = TOL_SMALL[22]
SHAPES = [(1, 1), (6, 40), (33, 64), (300, 64)]        # one ragged tile | ragged last tile, <= 2 splits | 66 tiles | test_gpu_round2's size


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"


def _spans(arch):
    """{(layer, 'W' | 'b'): (offset, out, in)} of the flat parameter vector."""
    out, off = {}, 0
    for name, o_, i_ in arch.layer_shapes():
        out[(name, "W")] = (off, o_, i_)
        off += o_ * i_
        out[(name, "b")] = (off, o_, 1)
        off += o_
    return out


def _part(arch, flat, name, part):
    off, o_, i_ = _spans(arch)[(name, part)]
    t = flat[off:off + o_ * i_]
    return t.reshape(o_, i_) if part == "W" else t


def _split_value(w):
    """float64 value of the (hi, lo) bf16 pair the split-bf16 streams hold for a float32 parameter."""
    hi = w.float().bfloat16().float()
    lo = (w.float() - hi).bfloat16().float()
    return hi.double() + lo.double()


def _partial_tail_bytes(m):
    """Bytes of the split-K partial-tile slots behind the dZ fragment blocks (csrc/mlp_frag.h: DW_PARTIAL_BYTES): 256 and 257
    samples differ by one 8-tile super-tile of fragment blocks."""
    from nerf_meets_mlx_amd import _native as N
    f = lambda M: N.lib().nerf_mlp_dz_bytes(C.byref(m.arch), M)
    return f(256) - (f(257) - f(256))


def _backward_poisoned(m, d_raw):
    """m.backward(d_raw) into NaN-filled grads, with the whole tail of the dz workspace (partial slots and scratch) NaN before."""
    from nerf_meets_mlx_amd import _native as N
    M = d_raw.numel() // 4
    nbytes = N.lib().nerf_mlp_dz_bytes(C.byref(m.arch), M)
    dz = m._workspace("dz", nbytes)
    tail = _partial_tail_bytes(m)
    assert 0 < tail < nbytes and tail % 4 == 0 and (nbytes - tail) % 4 == 0
    dz[nbytes - tail:nbytes].view(torch.float32).fill_(float("nan"))
    m.grads.fill_(float("nan"))
    return m.backward(d_raw).clone()


def _compare(tag, got, want):
    l2, mx = _rel_l2(got, want), _relmax(got, want)
    print(f"[dw_factor {tag}] rel-L2 {l2:.2e} rel-max {mx:.2e}")
    return l2, mx


@pytest.mark.parametrize("wgs", [0, 8])
@pytest.mark.parametrize("B,n", SHAPES)
def test_factored_gradients_against_the_stored_operands(B, n, wgs):
    """dW_F, db_F, dW_D[:, :256], dW_alpha, db_alpha of dw_factor 1 (and of dw_factor 0) against the float64 formulas on the stored
    operands; every other tensor of the two settings against each other; every element of grads written (NaN-filled before, with
    the dz workspace tail); two calls and the two launch orders bit-equal."""
    from nerf_meets_mlx_amd.models.NeRF import debug_layer
    m, arch, flat = _view(22)
    rays, z = _rays_z(B, n, 1000 * B + n)
    d_raw = torch.randn(B, n, 4, device=DEV, generator=torch.Generator(device=DEV).manual_seed(B + n))
    with options(dw_workgroups=wgs):
        m.query(rays, z, train=True)
        with options(dw_factor=1):
            g1 = _backward_poisoned(m, d_raw)
            g1_again = _backward_poisoned(m, d_raw)
            with options(dw_narrow_first=0):
                g1_wide_first = _backward_poisoned(m, d_raw)
        h7 = debug_layer(m, "acts", 7).double().cpu()
        dzd = debug_layer(m, "dz", 9).double().cpu()
        dza = debug_layer(m, "dz", 10)[:, 0].double().cpu()
        with options(dw_factor=0):
            g0 = _backward_poisoned(m, d_raw)
            with options(dw_narrow_first=0):
                g0_wide_first = _backward_poisoned(m, d_raw)
    assert bool(torch.isfinite(g1).all()), torch.nonzero(~torch.isfinite(g1)).flatten()[:8].tolist()
    assert bool(torch.isfinite(g0).all()), torch.nonzero(~torch.isfinite(g0)).flatten()[:8].tolist()
    assert torch.equal(g1, g1_again) and torch.equal(g1, g1_wide_first) and torch.equal(g0, g0_wide_first)
    # the reference: float64 on the host
    cpu = flat.cpu()
    WF, WD = _split_value(_part(arch, cpu, "feature", "W")), _split_value(_part(arch, cpu, "dir0", "W"))
    bF = _part(arch, cpu, "feature", "b").double()
    G, dbD = dzd.t() @ h7, dzd.sum(0)
    want = {("feature", "W"): WD[:, :256].t() @ G, ("feature", "b"): WD[:, :256].t() @ dbD,
            ("dir0", "W"): G @ WF.t() + torch.outer(dbD, bF),
            ("alpha", "W"): (dza[None, :] @ h7), ("alpha", "b"): dza.sum().reshape(1)}
    g1c, g0c = g1.cpu(), g0.cpu()
    for (name, part), ref in want.items():
        for setting, g in ((1, g1c), (0, g0c)):
            got = _part(arch, g, name, part)
            if name == "dir0":
                got = got[:, :256]
            l2, mx = _compare(f"{setting} {name}.{part} B={B} n={n} wgs={wgs}", got, ref)
            assert l2 <= TOL["dw"] and mx <= TOL["dw_max"], (setting, name, part, l2, mx)
    # everything else, dir0's direction columns among it: the two settings against each other
    for (name, part), (off, o_, i_) in _spans(arch).items():
        a, b = _part(arch, g1c, name, part), _part(arch, g0c, name, part)
        if (name, part) == ("dir0", "W"):
            a, b = a[:, 256:], b[:, 256:]
        elif (name, part) in want:
            continue
        l2, mx = _rel_l2(a, b), _relmax(a, b)
        assert l2 <= TOL["dw"] and mx <= TOL["dw_max"], (name, part, l2, mx)


def test_a_nan_upstream_gradient_travels_as_in_the_unfactored_path():
    """One NaN in d_raw (a colour channel of one sample) makes dW_F and db_F all NaN.  dW_D[:, :256]: the chain multiplies dZ_D with the
    ReLU decisions of dir0 as integers (csrc/mlp_frag.h: keep_where), so the rows of units that are off for that sample stay finite in
    the unfactored path; a row of G follows its row of dZ_D, so the factored path must poison exactly the same rows, each of them
    whole, and at least one."""
    m, arch, _ = _view(22)
    B, n = 6, 40
    rays, z = _rays_z(B, n, 5)
    d_raw = torch.randn(B, n, 4, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9))
    d_raw[3, 17, 1] = float("nan")
    m.query(rays, z, train=True)
    pats = {}
    for setting in (0, 1):
        with options(dw_factor=setting):
            g = m.backward(d_raw).cpu().clone()
        assert bool(torch.isnan(_part(arch, g, "feature", "W")).all()) and bool(torch.isnan(_part(arch, g, "feature", "b")).all()), setting
        pats[setting] = torch.isnan(_part(arch, g, "dir0", "W")[:, :256])
        rows = pats[setting].all(1)
        print(f"[dw_factor {setting}] NaN rows of dW_D[:, :256]: {int(rows.sum())} of 128")
        assert torch.equal(pats[setting], rows[:, None].expand(-1, 256)) and bool(rows.any()), setting
    assert torch.equal(pats[0], pats[1])


def test_trainer_moves_no_further_than_between_precisions():
    """20 Trainer.train_step iterations (N_rand 256, 100 x 100 images, seed 4).  d01 = parameter distance between dw_factor 0 and 1 at
    precision 22, d_prec = between precision 22 (dw_factor 0) and precision 32 of the same run: two accepted modes of one build.
    d01 <= d_prec per buffer (max-abs); all losses finite."""
    from nerf_meets_mlx_amd.dataset import synthetic
    from nerf_meets_mlx_amd.engine.trainer import Trainer
    imgs, poses, _, _, K = synthetic.make_dataset(100, 100, 4, seed=0, device=DEV)

    def run(precision, factor):
        with options(dw_factor=factor):
            tr = Trainer(imgs, poses, K, N_rand=256, seed=4, device=DEV, precision=precision)
            losses = [tr.train_step() for _ in range(20)]
            torch.cuda.synchronize()
            assert all(bool(torch.isfinite(v)) for out in losses for v in out.values()), (precision, factor)
            return {"coarse": tr.coarse.params.detach().clone(), "fine": tr.fine.params.detach().clone()}
    p0, p1, p32 = run(22, 0), run(22, 1), run(32, 0)
    for k in p0:
        d01 = float((p0[k] - p1[k]).abs().max())
        d_prec = float((p0[k] - p32[k]).abs().max())
        print(f"[dw_factor trainer] {k}: d01 {d01:.3e} d_prec {d_prec:.3e}")
        assert d01 <= d_prec, (k, d01, d_prec)
