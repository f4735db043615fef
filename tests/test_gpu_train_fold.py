"""The split-bf16 ("precision 22") TRAINING kernels with the feature layer folded into dir0 (csrc/mlp_s16.h, `NeRF.train_fold`,
`nerf_set_option("train_fold", 1)`).

`feature = W_F h7 + b_F` has no activation and only feeds dir0's first 256 input columns, so the folded image carries
W' = W_D[:, :256] W_F and b' = W_D[:, :256] b_F + b_D (float64 sums in index order, rounded once to float32): the training forward
runs dir0' on [h7 | direction encoding] and neither computes nor stores `feature`, the chain goes from [dZ_D | d alpha] to dZ7 through
[W'^T | W_A^T] and neither computes nor stores dZ_F, and the post step of the factored weight gradients forms dW_F, db_F and
dW_D[:, :256] from G = dZ_D^T H7 = dL/dW' and the fp32 masters by the product rule.

The view model of tests/test_gpu_f22_fold.py (b_F and b_D seeded N(0, 0.1), so that b' matters), in both input forms (rays + depths,
embedded rows) at: one sample; 33 (a ragged second tile); 2 x 128 x 2 + 33 = 545 with two persistent workgroups (the third pass of a
workgroup, a ragged last pass), pass queue on and off.  Every launch of a case runs once (module cache) and is shared by the tests:

  forward    raw and every stored activation that still exists against the float64 oracle at the fixture tolerance (1e-4 of the
             output scale); alpha and pos0..7 bit-identical to the unfolded form
  chain      dZ_D, d alpha, dZ_rgb bit-identical to the unfolded form; dZ7..dZ0 against the float64 chain on the kernel's own ReLU
             decisions at the bar of tests/test_gpu_round4.py / test_gpu_round5.py for the unfolded chain (rel-L2 1e-4)
  gradients  all 24 tensors against the float64 formulas on the stored operands and the fp32 masters, rel-L2 <= 1e-4
             (tests/test_gpu_dw_factor.py's bound)
  then: same W' and b' -> same bits; poisoned workspaces; non-finite inputs; 20 Trainer steps; checkpoint continuation.
"""
import pytest
import torch

from oracle import nerf_oracle as O
from tests._poison import NAN_BYTES, backward_into, forward_into, query_into, unwritten
from tests.test_gpu_f22_fold import _b, _base_flat, _rays_z, _spans, _w
from tests.test_gpu_pass_coverage import TOL, TOL_SMALL, _rel_l2, _relmax, _rows, options

pytestmark = pytest.mark.gpu
DEV = "cuda"
FWD_TOL = TOL[22]["fwd"]                       # 1e-4 of the output scale
DZ_TOL = TOL[22]["dz"]                         # 1e-4 rel-L2
DW_TOL = TOL_SMALL[22]["dw"]                   # 1e-4 rel-L2 (tests/test_gpu_dw_factor.py)
# (M, B, n, ring_workgroups, pass_queue)
CASES = [(1, 1, 1, 0, 1), (33, 11, 3, 0, 1), (545, 109, 5, 2, 1), (545, 109, 5, 2, 0)]
FORMS = ["rays", "rows"]
KEPT = [0, 1, 2, 3, 4, 5, 6, 7, 9]             # nerf_mlp_debug_read layers a folded model still stores: pos0..7, dir0
NAMES = {**{l: f"pos{l}" for l in range(8)}, 8: "feature", 9: "dir0"}
# fragment slots per 32-sample tile (csrc/mlp_layout.h, csrc/mlp_s16.h): the feature / dZ_F blocks, hi and lo
A_SLOTS, A_FEAT, A_LO = 325, 134, 158
Z_SLOTS, Z_F, Z_LO = 308, 128, 154


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"


def _model(flat, fold):
    from nerf_meets_mlx_amd.models.NeRF import NeRF
    m = NeRF(channel_input=63, channel_input_views=27, is_use_view_directions=True, device=DEV, seed=0, precision=22)
    m.load_flat(flat)
    m.train_fold = bool(fold)
    return m


_INPUTS, _RUNS, _ORACLE = {}, {}, {}


def _inputs(M, B, n):
    if M not in _INPUTS:
        rays, z = _rays_z(B, n, 2000 + M)
        rays, z = rays.to(DEV), z.to(DEV)
        x = _rows(rays, z).reshape(-1, 90).contiguous()
        d_raw = torch.randn(M, 4, device=DEV, generator=torch.Generator(device=DEV).manual_seed(M))
        _INPUTS[M] = (rays, z, x, d_raw)
    return _INPUTS[M]


def _run(case, form, fold):
    """One train-mode forward + backward of the case: raw, the stored activations and dZ (row-major float32), the gradients."""
    from nerf_meets_mlx_amd.models.NeRF import debug_layer
    key = (case, form, fold)
    if key not in _RUNS:
        M, B, n, wgs, pq = case
        rays, z, x, d_raw = _inputs(M, B, n)
        m = _model(_base_flat(O.NerfArch()), fold)
        with options(ring_workgroups=wgs, pass_queue=pq):
            raw = (m.query(rays, z, train=True) if form == "rays" else m.forward(x, train=True)).reshape(-1, 4).clone()
            assert m._packed_form == int(fold) and m._acts_form == int(fold)
            grads = m.backward(d_raw).clone()
        layers = KEPT if fold else KEPT + [8]
        r = {"raw": raw, "grads": grads,
             "acts": {l: debug_layer(m, "acts", l) for l in layers + [10, 11]},
             "dz": {l: debug_layer(m, "dz", l) for l in layers + [10, 11]}}
        if fold:
            with pytest.raises(ValueError, match="folded"):
                debug_layer(m, "acts", 8)
        torch.cuda.synchronize()
        _RUNS[key] = r
    return _RUNS[key]


def _oracle(case, form):
    """float64 oracle of the case on the FOLDED run's own ReLU decisions: outputs, taps and dL/d(tap)."""
    key = (case, form)
    if key not in _ORACLE:
        M, B, n, _, _ = case
        _, _, x, d_raw = _inputs(M, B, n)
        arch = O.NerfArch()
        r = _run(case, form, True)
        masks = {NAMES[l]: r["acts"][l] > 0 for l in KEPT}
        fl = _base_flat(arch).to(DEV).double().requires_grad_(True)
        p = O.unflatten_params(arch, fl)
        with torch.no_grad():
            free = O.nerf_forward(arch, p, x.double())
        taps = {}
        out = O.nerf_forward(arch, p, x.double().clone(), masks=masks, taps=taps)
        for t in taps.values():
            t.retain_grad()
        (out * d_raw.double()).sum().backward()
        _ORACLE[key] = (free, {k: v.detach() for k, v in taps.items()}, {k: v.grad for k, v in taps.items()}, masks)
    return _ORACLE[key]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"M{c[0]}-wgs{c[3]}-pq{c[4]}")
def test_folded_forward_against_the_oracle_and_the_unfolded_form(case, form):
    M = case[0]
    f, u = _run(case, form, True), _run(case, form, False)
    want, taps, _, _ = _oracle(case, form)
    _, _, x, _ = _inputs(*case[:3])
    assert bool(torch.isfinite(f["raw"]).all())
    e = _relmax(f["raw"], want)
    print(f"[train_fold M={M} {form}] raw {e:.3e} of the output scale (unfolded {_relmax(u['raw'], want):.3e})")
    assert e < FWD_TOL, e
    for l in KEPT:
        ea = float((f["acts"][l].double() - taps[NAMES[l]]).abs().max() / taps[NAMES[l]].abs().max().clamp_min(1e-300))
        print(f"[train_fold M={M} {form}] stored {NAMES[l]} {ea:.3e}")
        assert f["acts"][l].shape == taps[NAMES[l]].shape and ea < FWD_TOL, (NAMES[l], ea)
    pe, dpe = f["acts"][10], f["acts"][11]
    assert _relmax(pe[:, :63], x[:, :63]) < FWD_TOL and float(pe[:, 63:].abs().max()) == 0.0
    assert _relmax(dpe[:, :27], x[:, 63:]) < FWD_TOL and float(dpe[:, 27:].abs().max()) == 0.0
    # nothing upstream of dir0' changed: alpha and pos0..7 (and both encodings) bit for bit
    assert torch.equal(f["raw"][:, 3].view(torch.int32), u["raw"][:, 3].view(torch.int32))
    for l in list(range(8)) + [10, 11]:
        assert torch.equal(f["acts"][l].view(torch.int32), u["acts"][l].view(torch.int32)), l
    assert _relmax(f["raw"], u["raw"]) < FWD_TOL and _relmax(f["acts"][9], u["acts"][9]) < FWD_TOL


@pytest.mark.parametrize("form", FORMS)
def test_pass_queue_changes_no_bit_of_the_folded_form(form):
    a, b = _run(CASES[2], form, True), _run(CASES[3], form, True)
    assert torch.equal(a["raw"].view(torch.int32), b["raw"].view(torch.int32))
    assert torch.equal(a["grads"].view(torch.int32), b["grads"].view(torch.int32))
    for kind in ("acts", "dz"):
        for l in a[kind]:
            assert torch.equal(a[kind][l].view(torch.int32), b[kind][l].view(torch.int32)), (kind, l)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"M{c[0]}-wgs{c[3]}-pq{c[4]}")
def test_folded_chain_against_the_unfolded_form_and_the_float64_chain(case, form):
    M = case[0]
    f, u = _run(case, form, True), _run(case, form, False)
    _, _, dtaps, masks = _oracle(case, form)
    for l, what in ((9, "dZ_D"), (10, "d alpha"), (11, "dZ_rgb")):
        assert torch.equal(f["dz"][l].view(torch.int32), u["dz"][l].view(torch.int32)), what
    for l in range(7, -1, -1):
        ref = dtaps[NAMES[l]] * masks[NAMES[l]].double()
        e = _rel_l2(f["dz"][l], ref)
        print(f"[train_fold M={M} {form}] dZ{l} rel-L2 {e:.3e} (unfolded, on its own decisions' oracle: see test_gpu_round4)")
        assert e < DZ_TOL, (l, e)
    ref = dtaps["dir0"] * masks["dir0"].double()
    assert _rel_l2(f["dz"][9], ref) < DZ_TOL


def _formula_grads(arch, flat, r, x):
    """The 24 gradient tensors in float64 from the operands the kernels stored and the fp32 masters: {(layer, part): tensor}."""
    sp = _spans(arch)
    A = {l: t.double() for l, t in r["acts"].items()}
    Z = {l: t.double() for l, t in r["dz"].items()}
    pe, dpe = A[10][:, :63], A[11][:, :27]
    want = {}
    for l in range(8):
        h_in = pe if l == 0 else torch.cat([pe, A[4]], 1) if l == 5 else A[l - 1]
        want[(f"pos{l}", "W")], want[(f"pos{l}", "b")] = Z[l].t() @ h_in, Z[l].sum(0)
    WF, WD1, bF = _w(flat, sp, "feature").double(), _w(flat, sp, "dir0")[:, :256].double(), _b(flat, sp, "feature").double()
    G, dbD = Z[9].t() @ A[7], Z[9].sum(0)                      # G = dL/dW'
    want[("feature", "W")], want[("feature", "b")] = WD1.t() @ G, WD1.t() @ dbD
    want[("dir0", "W")] = torch.cat([G @ WF.t() + torch.outer(dbD, bF), Z[9].t() @ dpe], 1)
    want[("dir0", "b")] = dbD
    want[("alpha", "W")], want[("alpha", "b")] = Z[10][:, :1].t() @ A[7], Z[10][:, 0].sum().reshape(1)
    want[("rgb", "W")], want[("rgb", "b")] = Z[11][:, :3].t() @ A[9], Z[11][:, :3].sum(0)
    return want


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"M{c[0]}-wgs{c[3]}-pq{c[4]}")
def test_folded_gradients_against_the_stored_operands_and_the_masters(case, form):
    arch = O.NerfArch()
    sp = _spans(arch)
    flat = _base_flat(arch).to(DEV)
    r = _run(case, form, True)
    assert bool(torch.isfinite(r["grads"]).all())
    want = _formula_grads(arch, flat, r, _inputs(*case[:3])[2])
    assert len(want) == 24
    worst = (0.0, None)
    for (name, part), ref in want.items():
        got = (_w if part == "W" else _b)(r["grads"], sp, name)
        if float(ref.norm()) == 0.0:
            assert float(got.abs().max()) == 0.0, (name, part)
            continue
        e = _rel_l2(got, ref)
        print(f"[train_fold M={case[0]} wgs={case[3]} {form}] d{name}.{part} rel-L2 {e:.3e}")
        worst = max(worst, (e, (name, part)))
        assert e <= DW_TOL, (name, part, e)
    print(f"[train_fold M={case[0]} wgs={case[3]} {form}] worst {worst[0]:.3e} at {worst[1]} (bar {DW_TOL:.0e})")


def test_same_folded_weights_give_the_same_bits():
    """Two parameter sets with exactly the same W' and b' (a scaled permutation as W_F): same raw, same dZ7 -- pins the product's
    orientation, its element order and the single rounding, in both streams."""
    from nerf_meets_mlx_amd.models.NeRF import debug_layer
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
    rays, z, x, d_raw = _inputs(*CASES[1][:3])
    got = []
    for flat in (flat_a, flat_b):
        m = _model(flat, True)
        raw = m.query(rays, z, train=True).clone()
        m.backward(d_raw)
        got.append((raw, debug_layer(m, "dz", 7).clone(), debug_layer(m, "acts", 9).clone()))
    (ra, za, ha), (rb, zb, hb) = got
    assert bool(torch.isfinite(ra).all()) and float(ra[..., :3].abs().max()) > 0 and float(za.abs().max()) > 0
    assert torch.equal(ra.view(torch.int32), rb.view(torch.int32)), int((ra.view(torch.int32) != rb.view(torch.int32)).sum())
    assert torch.equal(ha.view(torch.int32), hb.view(torch.int32))
    assert torch.equal(za.view(torch.int32), zb.view(torch.int32)), int((za.view(torch.int32) != zb.view(torch.int32)).sum())


@pytest.mark.parametrize("form", FORMS)
def test_poisoned_workspaces_leave_the_feature_slots_alone(form):
    """acts, dz and grads NaN-filled before the launches: every output and gradient is written and finite, equal to the clean run bit
    for bit, and the A_FEAT / Z_F blocks (hi and lo) of every tile still hold the poison: nothing wrote them, so nothing read them."""
    case = CASES[2]
    M, B, n, wgs, pq = case
    rays, z, x, d_raw = _inputs(M, B, n)
    clean = _run(case, form, True)
    m = _model(_base_flat(O.NerfArch()), True)
    with options(ring_workgroups=wgs, pass_queue=pq, train_fold=1):
        raw = query_into(m, rays, z, NAN_BYTES, train=True) if form == "rays" else forward_into(m, x, NAN_BYTES, train=True)
        grads = backward_into(m, d_raw, NAN_BYTES).clone()
    assert m._packed_form == 1
    assert unwritten(raw) == 0 and unwritten(grads) == 0
    assert bool(torch.isfinite(raw).all()) and bool(torch.isfinite(grads).all())
    assert torch.equal(raw.reshape(-1, 4), clean["raw"]) and torch.equal(grads, clean["grads"])
    tiles = ((M + 31) // 32 + 7) // 8 * 8
    acts = m._ws["acts"][:tiles * A_SLOTS * 1024].view(tiles, A_SLOTS, 1024)
    dz = m._ws["dz"][:tiles * Z_SLOTS * 1024].view(tiles, Z_SLOTS, 1024)
    for lo in (0, A_LO):
        assert bool((acts[:, lo + A_FEAT:lo + A_FEAT + 16] == NAN_BYTES).all()), "the forward wrote a feature block"
    for lo in (0, Z_LO):
        assert bool((dz[:, lo + Z_F:lo + Z_F + 16] == NAN_BYTES).all()), "the chain wrote a dZ_F block"
    live = (M + 31) // 32
    assert not bool((acts[:live, A_FEAT - 16:A_FEAT] == NAN_BYTES).all()) and not bool((dz[:live, Z_F - 16:Z_F] == NAN_BYTES).all())


@pytest.mark.parametrize("form", FORMS)
def test_non_finite_inputs_travel_as_in_the_unfolded_form(form):
    """A NaN position makes all four outputs of its samples NaN, a NaN direction the three colours (alpha bit-identical to the clean
    run), every other sample bit-identical to the clean run."""
    case = CASES[1]
    M, B, n, _, _ = case
    rays, z, x, _ = _inputs(M, B, n)
    clean = _run(case, form, True)["raw"]
    m = _model(_base_flat(O.NerfArch()), True)
    for what in ("position", "direction"):
        if form == "rays":
            bad = rays.clone()
            bad[4, 1 if what == "position" else 9] = float("nan")        # origin | view direction of ray 4: samples 12..14
            hit = torch.zeros(M, dtype=torch.bool, device=DEV)
            hit[4 * n:5 * n] = True
            got = m.query(bad, z, train=True).reshape(-1, 4)
        else:
            bad = x.clone()
            bad[17, 5 if what == "position" else 70] = float("nan")
            hit = torch.zeros(M, dtype=torch.bool, device=DEV)
            hit[17] = True
            got = m.forward(bad, train=True)
        assert bool(torch.isnan(got[hit, :3]).all()), what
        if what == "position":
            assert bool(torch.isnan(got[hit, 3]).all())
        else:
            assert torch.equal(got[hit, 3].view(torch.int32), clean[hit, 3].view(torch.int32))
        assert torch.equal(got[~hit].view(torch.int32), clean[~hit].view(torch.int32)), what


def test_a_nan_in_w_f_poisons_every_colour_and_no_alpha():
    arch = O.NerfArch()
    sp = _spans(arch)
    case = CASES[1]
    rays, z, _, _ = _inputs(*case[:3])
    clean = _run(case, "rays", True)["raw"]
    bad = _base_flat(arch)
    _w(bad, sp, "feature")[77, 130] = float("nan")
    got = _model(bad, True).query(rays, z, train=True).reshape(-1, 4)
    assert bool(torch.isnan(got[:, :3]).all())
    assert torch.equal(got[:, 3].view(torch.int32), clean[:, 3].view(torch.int32))


def _trainer(precision, fold, data):
    from nerf_meets_mlx_amd.engine.trainer import Trainer
    imgs, poses, K = data
    tr = Trainer(imgs, poses, K, N_rand=256, seed=4, device=DEV, precision=precision)
    assert tr.coarse.train_fold and tr.fine.train_fold          # the Trainer asks for the folded form (it takes effect at precision 22)
    tr.coarse.train_fold = tr.fine.train_fold = bool(fold)
    return tr


def test_trainer_moves_no_further_than_between_precisions_and_continues_bit_identically(tmp_path):
    """20 Trainer.train_step iterations (N_rand 256, 100 x 100 images, seed 4), folded against unfolded at precision 22: the parameters
    move no further apart (max-abs per buffer) than precision 22 (unfolded) does from precision 32 -- the yardstick of
    tests/test_gpu_dw_factor.py::test_trainer_moves_no_further_than_between_precisions.  A checkpoint written after 3 folded steps
    and loaded into a fresh trainer continues bit-identically."""
    from nerf_meets_mlx_amd.dataset import synthetic
    imgs, poses, _, _, K = synthetic.make_dataset(100, 100, 4, seed=0, device=DEV)
    data = (imgs, poses, K)

    def run(precision, fold):
        tr = _trainer(precision, fold, data)
        losses = [tr.train_step() for _ in range(20)]
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(v)) for out in losses for v in out.values()), (precision, fold)
        assert tr.coarse._packed_form == tr.fine._packed_form == int(bool(fold) and precision == 22)
        return {"coarse": tr.coarse.params.detach().clone(), "fine": tr.fine.params.detach().clone()}
    p0, p1, p32 = run(22, False), run(22, True), run(32, False)
    for k in p0:
        d01 = float((p0[k] - p1[k]).abs().max())
        d_prec = float((p0[k] - p32[k]).abs().max())
        print(f"[train_fold trainer] {k}: d01 {d01:.3e} d_prec {d_prec:.3e}")
        assert d01 <= d_prec, (k, d01, d_prec)
    a = _trainer(22, True, data)
    for _ in range(3):
        a.train_step()
    a.save(str(tmp_path / "ck"))
    b = _trainer(22, True, data)
    assert b.load(str(tmp_path / "ck")) == 3
    for _ in range(2):
        a.train_step()
        b.train_step()
    assert a.coarse._packed_form == 1 and b.fine._packed_form == 1
    for k, ma in a._checkpoint_buffers().items():
        assert torch.equal(ma.params, b._checkpoint_buffers()[k].params), k
