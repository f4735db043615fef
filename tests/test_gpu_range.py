"""The MLP kernels on exponent-shifted weights (tests/_range_ref.py: `rescale`, the families "act" and "alt", shift k = log2 of the scale).

Every other MLP test runs at one operating point (weights init x 1.5 or randn x 0.05, activations of order 1).  Here the same
function is computed with the hidden layers' scales moved by 2^k, which changes no bit of the float64 oracle
(tests/test_range_host.py) and moves the magnitude of every operand the kernels see.

a. Split-fp16 inference (csrc/mlp22.hip; view model, precision 22, query(train=False), f22_tiles 2 and 3), B = 5 rays x n = 97 depths
   (485 samples: two passes of the 48-sample form and a ragged tail), against the float64 oracle, error relative to the output scale:
     window    |k| in {4, 7}:          every output finite, error <= 1e-4 (TOL[22]["fwd"], the bar of every other forward test);
     degraded  |k| in {8, 10, 12, 14}: every output finite, error <= E_EMU(family, k) + 1e-4: the CPU emulation of the kernel's
               operand formats (tests/_range_ref.py `emulate22`, table asserted by tests/test_range_host.py) gives the representation
               error -- weights below 2^-14 carry 11 bits -- and the bar covers what it leaves out (fp32 accumulation order, the
               kernel's own sine);
     overflow  `act` +15, `act` +18, `alt` -20 (weights x 2^20): every output ELEMENT is non-finite or within the degraded bound --
               never a silent wrong value -- and at the last two every output is non-finite, as the emulation says.  The row-by-row
               finite pattern at +15 is not compared: values between 65504 and 65520 round either way.
   The window's edge is 7, not the 8 first supposed: the faithful emulation (no lo.lo term) gives 1.3e-5 at |k| = 8, above one tenth of
   the bar (tests/test_range_host.py), so +-8 is held to the degraded bound.
   What this would catch (shown on the emulation in tests/test_range_host.py): a matrix unit that flushed subnormal fp16 inputs
   (1.9e-2 at `act` -8, 4e-4 at -4), a conversion that saturated at 65504 (finite outputs at +18, 0.27 off).

b. The paths that carry float32's exponent range -- split-bf16 training at precision 22 (csrc/mlp_s16.hip, mlp_s16f.hip, mlp_dww.hip,
   mlp_dwf.hip; "train_fold" 0 and 1), bf16 at 16 (csrc/mlp.hip), fp32 at 32 (csrc/mlp32.hip), the image and 2 x 64 models
   (csrc/mlp_s16x.hip, mlp.hip) -- at k = -20 and +20, both families, with sentinel outputs and poisoned workspaces (tests/_poison.py):
     * forward, dW / db (and dL/dx of the 2 x 64 model) against the oracle of the RESCALED parameters on the kernel's own ReLU
       decisions, at the bars of TOL / TOL_SMALL for that path (the bf16-emulating oracle at 16);
     * the forward output is bit-identical to the same call at k = 0: bf16 / fp32 rounding, fp32 accumulation, the bias add and ReLU
       all commute with an exact power of two while nothing is subnormal;
     * the kernel's ReLU decisions (stored activation > 0) are those of k = 0;
     * beyond what was asked: the gradients, mapped back with dW_l = dW_l' c_l / c_in, and dL/dx are bit-identical to k = 0 too (the
       bf16 / fp32 rounding of dZ, the fp32 accumulation of dW and the float64 post step of the factored jobs commute with a power
       of two in the same way; measured 0 differing elements on every path before it was made an assertion).
   View model: B = 5, n = 97 through query(); image and 2 x 64 models: M = 65 embedded rows (two tiles and a one-sample tail).
"""
import pytest
import torch

from tests import _range_ref as R
from tests._poison import BIG_BYTES, NAN_BYTES, backward_into, bits_equal, forward_into, layer_into, query_into, unwritten
from tests.test_gpu_pass_coverage import (LAYER_NAMES, TOL, TOL_SMALL, _check_grads, _image, _oracle_backward, _oracle_forward, _rays_z,
                                          _rel_l2, _relmax, _rows, _small, _view, options)

pytestmark = pytest.mark.gpu
DEV = "cuda"
_MODELS, _INPUTS, _BASE = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"


def _model(kind, precision):
    """One model per (kind, precision) for the module: (model, arch, unshifted flat parameters on the device)."""
    if (kind, precision) not in _MODELS:
        m, arch, flat = {"view": _view, "image": _image, "small": _small}[kind](precision)
        want_arch, want = R.model_flat(kind)
        assert torch.equal(flat.cpu(), want) and arch.layer_shapes() == want_arch.layer_shapes()
        _MODELS[(kind, precision)] = (m, arch, flat)
    return _MODELS[(kind, precision)]


def _view_inputs():
    if "view" not in _INPUTS:
        rays, z = _rays_z(R.B_RAYS, R.N_DEPTHS, R.SEED)
        rc, zc = R.rays_z(R.B_RAYS, R.N_DEPTHS, R.SEED)                   # the inputs of the committed emulation table
        assert torch.equal(rays.cpu(), rc) and torch.equal(z.cpu(), zc)
        d = torch.randn(R.B_RAYS, R.N_DEPTHS, 4, generator=torch.Generator().manual_seed(1)).to(DEV)
        _INPUTS["view"] = (rays, z, _rows(rays, z), d)
    return _INPUTS["view"]


def _row_inputs(kind):
    if kind not in _INPUTS:
        x, d = R.row_inputs(kind)
        _INPUTS[kind] = (x.to(DEV), d.to(DEV))
    return _INPUTS[kind]


def _shifted(arch, flat, family, k):
    return R.rescale(arch, flat, R.scales(arch, family, k))


# ------------------------------------------------------------------------------------------------ a. split-fp16 inference
def _infer22(family, k, tiles):
    """(raw [485, 4], float64 oracle of the shifted parameters) of the split-fp16 inference forward."""
    m, arch, flat = _model("view", 22)
    rays, z, x, _ = _view_inputs()
    fk = _shifted(arch, flat, family, k)
    m.load_flat(fk)
    with options(f22_tiles=tiles):
        raw = query_into(m, rays, z, NAN_BYTES)
    assert unwritten(raw) == 0, (family, k, tiles, unwritten(raw))
    return raw.reshape(-1, 4), _oracle_forward(arch, fk, x, False)


@pytest.mark.parametrize("k", [s * k for k in R.WINDOW for s in (1, -1)])
@pytest.mark.parametrize("family", R.FAMILIES)
def test_split_fp16_inference_inside_the_window(family, k):
    for tiles in (2, 3):
        got, want = _infer22(family, k, tiles)
        assert bool(torch.isfinite(got).all()), (family, k, tiles)
        e = _relmax(got, want)
        print(f"[range 22 inference {family} k={k:+d} f22_tiles={tiles}] {e:.3e} of the output scale (bar {TOL[22]['fwd']:.0e}, "
              f"emulation {R.E_EMU[(family, k)]:.2e})")
        assert e <= TOL[22]["fwd"], (family, k, tiles, e)


@pytest.mark.parametrize("k", [s * k for k in R.DEGRADED for s in (1, -1)])
@pytest.mark.parametrize("family", R.FAMILIES)
def test_split_fp16_inference_degraded(family, k):
    bound = R.degraded_bound(family, k)
    assert bound == R.E_EMU[(family, k)] + TOL[22]["fwd"]
    for tiles in (2, 3):
        got, want = _infer22(family, k, tiles)
        assert bool(torch.isfinite(got).all()), (family, k, tiles)
        e = _relmax(got, want)
        print(f"[range 22 inference {family} k={k:+d} f22_tiles={tiles}] {e:.3e} of the output scale (bound {bound:.3e} = emulation "
              f"{R.E_EMU[(family, k)]:.3e} + {TOL[22]['fwd']:.0e})")
        assert e <= bound, (family, k, tiles, e, bound)


@pytest.mark.parametrize("family,k", R.OVERFLOW, ids=[f"{f}{k:+d}" for f, k in R.OVERFLOW])
def test_split_fp16_inference_overflow_is_never_silent(family, k):
    bound = R.degraded_bound(family, k)
    for tiles in (2, 3):
        got, want = _infer22(family, k, tiles)
        finite = torch.isfinite(got)
        err = (got.double() - want).abs() / want.abs().max()
        worst = float(err[finite].max()) if bool(finite.any()) else 0.0
        print(f"[range 22 inference {family} k={k:+d} f22_tiles={tiles}] finite rows {int(finite.all(-1).sum())} of {got.shape[0]}, "
              f"finite elements {int(finite.sum())}, worst finite element {worst:.3e} of the output scale (bound {bound:.3e})")
        assert worst <= bound, (family, k, tiles, worst, bound)
        if k != 15:
            assert not bool(finite.any()), (family, k, tiles, int(finite.sum()))


# ------------------------------------------------------------------------------------------------ b. float32-exponent paths
PATHS = [("view", 22, 0), ("view", 22, 1), ("view", 16, 0), ("view", 32, 0), ("image", 22, 0), ("image", 16, 0), ("small", 22, 0),
         ("small", 16, 0)]                                                # (model, precision, "train_fold")
MASK_LAYERS = {"view": [(l, n) for l, n in enumerate(LAYER_NAMES) if n != "feature"], "image": [(l, f"pos{l}") for l in range(8)],
               "small": [(0, "pos0"), (1, "pos1"), (9, "dir0")]}


def _run(kind, precision, fold, fk):
    """Inference forward (where it runs the same kernels' arithmetic: not the view model at 22, whose inference is part a), training
    forward and backward on parameters fk under both workspace patterns: {"inf", "trn", "grads", "dx", "acts": {name: [M, width]}}."""
    m, arch, _ = _model(kind, precision)
    m.load_flat(fk)
    m.train_fold = bool(fold)
    res = {}
    opts = dict(train_fold=fold) if (kind == "view" and precision == 22) else {}
    with options(**opts):
        for pat in (BIG_BYTES, NAN_BYTES):
            r = {}
            if kind == "view":
                rays, z, _, d = _view_inputs()
                if precision != 22:
                    r["inf"] = query_into(m, rays, z, pat)
                r["trn"] = query_into(m, rays, z, pat, train=True)
                r["grads"] = backward_into(m, d, pat).clone()
            else:
                x, d = _row_inputs(kind)
                r["inf"] = forward_into(m, x, pat)
                r["trn"] = forward_into(m, x, pat, train=True)
                if kind == "small":
                    g, dx = backward_into(m, d, pat, need_input_grad=True)
                    r["grads"], r["dx"] = g.clone(), dx
                else:
                    r["grads"] = backward_into(m, d, pat).clone()
            for l, n in MASK_LAYERS[kind]:
                r["act_" + n] = layer_into(m, "acts", l)
            for key, t in r.items():
                assert unwritten(t) == 0, (kind, precision, fold, pat, key, unwritten(t))
            res[pat] = r
    assert m._packed_form == int(fold)
    for key in res[NAN_BYTES]:
        assert bits_equal(res[BIG_BYTES][key], res[NAN_BYTES][key]), (kind, precision, fold, "result depends on workspace contents", key)
    return res[NAN_BYTES]


def _base(kind, precision, fold):
    """The same calls at k = 0, once per path."""
    key = (kind, precision, fold)
    if key not in _BASE:
        _BASE[key] = _run(kind, precision, fold, _model(kind, precision)[2])
    return _BASE[key]


@pytest.mark.parametrize("k", [-20, 20])
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("kind,precision,fold", PATHS, ids=[f"{a}{p}" + ("-fold" if f else "") for a, p, f in PATHS])
def test_float32_exponent_paths_are_shift_invariant(kind, precision, fold, family, k):
    m, arch, flat = _model(kind, precision)
    tol = (TOL if kind == "view" else TOL_SMALL)[precision]
    tag = (kind, precision, fold, family, k)
    base = _base(kind, precision, fold)
    fk = _shifted(arch, flat, family, k)
    got = _run(kind, precision, fold, fk)
    if kind == "view":
        _, _, x, d = _view_inputs()
        d = d.reshape(-1, 4)
    else:
        x, d = _row_inputs(kind)
    # against the oracle of the rescaled parameters
    want = _oracle_forward(arch, fk, x, tol["emu"])
    fwd = {key: _relmax(got[key].reshape(want.shape), want) for key in ("inf", "trn") if key in got}
    masks = {n: got["act_" + n] > 0 for _, n in MASK_LAYERS[kind]}
    gw, gx = _oracle_backward(arch, fk, x, d, masks, tol["emu"], need_dx=(kind == "small"))
    e_dx = _rel_l2(got["dx"], gx) if kind == "small" else None
    print(f"[range {kind} p{precision} fold={fold} {family} k={k:+d}] forward " + ", ".join(f"{a} {e:.2e}" for a, e in fwd.items())
          + f" of the output scale (bar {tol['fwd']:.0e})" + (f", dL/dx rel-L2 {e_dx:.2e} (bar {tol['dx']:.0e})" if kind == "small" else ""))
    for key, e in fwd.items():
        assert e < tol["fwd"], (tag, key, e)
    worst = _check_grads(arch, got["grads"], gw, tol, tag)
    print(f"[range {kind} p{precision} fold={fold} {family} k={k:+d}] worst dW / db rel-L2 {worst:.2e} (bar {tol['dw']:.0e})")
    if kind == "small":
        assert e_dx < tol["dx"], (tag, e_dx)
    # against the same call at k = 0
    for key in fwd:
        diff = int((got[key].view(torch.int32) != base[key].view(torch.int32)).sum())
        assert bits_equal(got[key], base[key]), (tag, key, "forward differs from k = 0 in", diff, "elements")
    gb = R.grads_back(arch, got["grads"], R.scales(arch, family, k))
    gdiff = int((gb.view(torch.int32) != base["grads"].view(torch.int32)).sum())
    xdiff = int((got["dx"].view(torch.int32) != base["dx"].view(torch.int32)).sum()) if kind == "small" else 0
    print(f"[range {kind} p{precision} fold={fold} {family} k={k:+d}] gradients mapped back differ from k = 0 in {gdiff} of {gb.numel()} "
          f"elements, dL/dx in {xdiff}")
    assert gdiff == 0 and xdiff == 0, (tag, "the backward is not shift invariant", gdiff, xdiff)
    for _, n in MASK_LAYERS[kind]:
        flips =int(((got["act_" + n] > 0) != (base["act_" + n] > 0)).sum())
        assert flips == 0, (tag, n, "ReLU decisions differ from k = 0 in", flips, "units")
