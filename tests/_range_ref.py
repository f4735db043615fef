"""Exponent-shifted weights for the MLP kernels, and a CPU emulation of the split-fp16 inference forward (a helper module, not a
conftest; numpy / torch on the CPU only -- nothing here touches the device or the native library).

1. `rescale`: a power-of-two change of the hidden layers' activation scales that leaves the network's function unchanged.  With
   c[l] = 2^k the scale of hidden layer l (inputs and outputs keep scale 1),
       W_l' = W_l c_l / c_in(column),   b_l' = b_l c_l,
   where c_in is the scale of the layer that produces the column (1 for the columns that read network inputs: all of pos0, the skip
   layer's position columns, dir0's direction columns).  ReLU commutes with a positive scale and a power of two is exact in every
   binary format, so the float64 oracle of the rescaled parameters equals that of the original ones exactly, every hidden activation
   is the original one times c_l, and the gradients map back as dW_l = dW_l' c_l / c_in, db_l = db_l' c_l (`grads_back`).
   Two families (`scales`):  "act": every hidden layer 2^k -- moves the activations and the first and last weights;
                             "alt": hidden layers 0, 2, 4, .. 2^k, the others 1 -- moves the weights of every layer, alternately up and down.

2. `emulate22`: the split-fp16 ("precision 22") inference forward of the 8 x 256 view model as csrc/mlp22.hip states it:
     weights (pack22_kernel):  hi = 0 if |w| < 2^-14 else fp16(w);  lo = fp16((w - hi) 2^11)           (float32 arithmetic)
     layer inputs (split2):    hi = fp16(v) (round to nearest even, subnormals kept);  lo = fp16((v - hi) 2^11)
     product:                  v' = float32(b + hi.hi + 2^-11 (hi.lo + lo.hi)), no lo.lo term, fp32 bias, IEEE maximum(v', 0)
   with the sums taken in float64 (the kernel accumulates in float32: its order-dependent rounding is what the project's 1e-4 forward
   bar covers, not this emulation) on the oracle's float32 encodings (the kernel's own sine is within 6e-7 of them).  The folded
   stream (NERF_F22_FOLD 1, the build's default in csrc/mlp22.h; tests/test_range_host.py reads the header) has no feature layer:
   dir0 multiplies [h7, input_dir] with W' = float32(W_D[:, :256] W_F), b' = float32(W_D[:, :256] b_F + b_D), products and sums in
   float64 as in the packer.  A fp16 conversion overflows to inf at |v| >= 65520 and (inf - inf) makes the lo part NaN, as on the device.

3. `E_EMU`: the committed table of `emulate22`'s error against the float64 oracle, relative to the output scale, on the inputs of
   tests/test_gpu_range.py (`init(seed 3) x 1.5`, B = 5 rays x n = 97 depths, `rays_z(5, 97, SEED)`); tests/test_range_host.py asserts that
   the emulation reproduces it, tests/test_gpu_range.py builds the bounds of the degraded cases from it.
"""
import numpy as np
import torch

from oracle import nerf_oracle as O

SEED = 4242                     # inputs of the range tests: rays_z(B, N_DEPTHS, SEED)
B_RAYS, N_DEPTHS = 5, 97        # 485 samples: two passes of the 48-sample form of csrc/mlp22.hip and a ragged tail
FAMILIES = ("act", "alt")
WINDOW = (4, 7)                 # |k| inside the full-precision window: E_EMU <= 1e-5 (one tenth of the forward bar); 1.3e-5 at |k| = 8
DEGRADED = (8, 10, 12, 14)      # |k| at which every output is still finite and the error is the emulation's + the forward bar
OVERFLOW = (("act", 15), ("act", 18), ("alt", -20))        # the last two: every output non-finite
F16_MIN_NORMAL = 2.0 ** -14


# ------------------------------------------------------------------------------------------------ inputs
def rays_z(B, n, seed):
    """tests/test_gpu_pass_coverage.py `_rays_z` on the CPU (same generator, same draws)."""
    g = torch.Generator().manual_seed(seed)
    o = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=-1) * 4.0
    rays = O.pack_rays(o, -o / 4.0 + 0.25 * torch.randn(B, 3, generator=g), 2.0, 6.0)
    z = torch.sort(torch.rand(B, n, generator=g) * 4 + 2, -1).values
    return rays, z


def rows(rays, z):
    """tests/test_gpu_pass_coverage.py `_rows`: the reference's float32 inputs of the network, [B n, 90]."""
    pos = rays[:, None, 0:3] + z[..., None] * rays[:, None, 3:6]
    return O.embed(pos, rays[:, 8:11])


def view_flat(seed=3):
    """The parameters of tests/test_gpu_pass_coverage.py `_view`."""
    arch = O.NerfArch()
    return arch, O.flatten_params(arch, O.init_params(arch, seed)) * 1.5


M_ROWS = 65                     # embedded rows of the image and 2 x 64 models: two 32-sample tiles and a one-sample tail
KINDS = ("view", "image", "small")


def model_flat(kind):
    """(arch, flat) of tests/test_gpu_pass_coverage.py `_view / _image / _small` (tests/test_gpu_round5.py `_image_pair / _small_pair`)."""
    if kind == "view":
        return view_flat()
    arch = (O.NerfArch(channel_input=40, channel_input_views=0, channel_output=3, use_viewdirs=False) if kind == "image" else
            O.NerfArch(channel_input=32, channel_input_views=16, n_layers=2, width=64, skips=(), use_viewdirs=True))
    return arch, O.flatten_params(arch, O.init_params(arch, 0)) * 1.5


def row_inputs(kind):
    """(x [M_ROWS, in], d_out [M_ROWS, out]) of order 1 for the embedded-row entries."""
    arch, _ = model_flat(kind)
    gen = torch.Generator().manual_seed(M_ROWS)
    cin = arch.cin + (arch.cdir if arch.use_viewdirs else 0)
    return torch.randn(M_ROWS, cin, generator=gen), torch.randn(M_ROWS, 4 if arch.use_viewdirs else arch.cout, generator=gen)


# ------------------------------------------------------------------------------------------------ rescaling
def hidden_layers(arch):
    return [f"pos{i}" for i in range(arch.D)] + (["feature", "dir0"] if arch.use_viewdirs else [])


def scales(arch, family, k):
    """{hidden layer: 2^k or 1} of the family."""
    names = hidden_layers(arch)
    if family == "act":
        return {n: 2.0 ** k for n in names}
    assert family == "alt", family
    return {n: (2.0 ** k if i % 2 == 0 else 1.0) for i, n in enumerate(names)}


def factors(arch, c):
    """float64 flat vector f with W_l' = W_l f, b_l' = b_l f elementwise: c_l / c_in(column) for weights, c_l for biases."""
    last = f"pos{arch.D - 1}"
    out = []
    for name, o, i in arch.layer_shapes():
        cl = float(c.get(name, 1.0))                                     # alpha, rgb, output: network outputs, scale 1
        cin = torch.ones(i, dtype=torch.float64)
        if name.startswith("pos") and name != "pos0":
            l = int(name[3:])
            cin[:] = c[f"pos{l - 1}"]
            if (l - 1) in arch.skips:                                    # concat[input_pos, h]: the position columns come first
                assert i == arch.W + arch.cin
                cin[:arch.cin] = 1.0
        elif name in ("feature", "alpha", "output"):
            cin[:] = c[last]
        elif name == "dir0":                                             # concat[feature, input_dir]
            cin[:arch.W] = c["feature"]
        elif name == "rgb":
            cin[:] = c["dir0"]
        out += [(cl / cin).expand(o, i).reshape(-1), torch.full((o,), cl, dtype=torch.float64)]
    return torch.cat(out)


def rescale(arch, flat, c):
    """The flat parameter vector with hidden-layer activation scales c = {layer: 2^k} (exact: every factor is a power of two)."""
    f = factors(arch, c).to(flat.device)
    out = flat.double() * f
    assert bool((out.to(flat.dtype).double() == out).all()), "rescale: a parameter left the range of its format"
    return out.to(flat.dtype)


def grads_back(arch, grads, c):
    """Gradients with respect to the rescaled parameters -> gradients with respect to the original ones."""
    return (grads.double() * factors(arch, c).to(grads.device)).to(grads.dtype)


# ------------------------------------------------------------------------------------------------ split-fp16 emulation
def _f16(a):
    """float32 -> fp16 -> float64: round to nearest even, subnormals kept, |a| >= 65520 -> inf."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(a, np.float32).astype(np.float16).astype(np.float64)


def split_weight(w):
    """pack22_kernel: (hi, lo) of float32 weights as float64 arrays of fp16 values."""
    w = np.asarray(w, np.float32)
    hi = np.where(np.abs(w) < F16_MIN_NORMAL, 0.0, _f16(w))
    with np.errstate(over="ignore", invalid="ignore"):
        lo = _f16(((w - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float32))
    return hi, lo


def split_act(v, variant=None):
    """split2: (hi, lo) of float32 layer inputs.  variant (sensitivity checks of tests/test_range_host.py only):
    "flush": a subnormal hi is flushed to zero and the lo part computed from the unflushed hi (what a matrix unit that flushed
             subnormal fp16 inputs would make of the kernel's operands);
    "saturate": the hi conversion clamps at +-65504 where the kernel's overflows to inf."""
    v = np.asarray(v, np.float32)
    hi = _f16(v)
    if variant == "saturate":
        hi = np.where(np.isnan(v), hi, np.clip(hi, -65504.0, 65504.0))
    with np.errstate(over="ignore", invalid="ignore"):
        lo = _f16(((v.astype(np.float64) - hi) * 2048.0).astype(np.float32))          # v 2^11 - hi 2^11: exact, one fma in the kernel
    if variant == "saturate":
        lo = np.where(np.isnan(lo), lo, np.clip(lo, -65504.0, 65504.0))
    if variant == "flush":
        hi = np.where(np.abs(hi) < F16_MIN_NORMAL, 0.0, hi)
    return hi, lo


def _linear22(w, b, v, relu, variant):
    wh, wl = split_weight(w)
    ah, al = split_act(v, variant)
    with np.errstate(over="ignore", invalid="ignore"):
        main = b.astype(np.float64)[None, :] + ah @ wh.T
        corr = ah @ wl.T + al @ wh.T
        out = (main + corr / 2048.0).astype(np.float32)
    return np.maximum(out, np.float32(0.0)) if relu else out                           # IEEE maximum: NaN stays NaN


def emulate22_forward(arch, flat, x, fold=True, variant=None):
    """[M, 4] float32 = [rgb, alpha] raw of the emulated split-fp16 forward of the view model on embedded rows x [M, 90]."""
    assert arch.use_viewdirs and arch.skips == (4,) and arch.D == 8, "the split-fp16 inference kernel is the 8 x 256 view model's"
    p = {n: (w.numpy().astype(np.float32), b.numpy().astype(np.float32))
         for n, (w, b) in O.unflatten_params(arch, flat.detach().cpu().float()).items()}
    x = x.detach().cpu().float().numpy()
    xp, xd = x[:, :arch.cin], x[:, arch.cin:]
    h = xp
    for i in range(arch.D):
        h = _linear22(*p[f"pos{i}"], h, True, variant)
        if i in arch.skips:
            h = np.concatenate([xp, h], -1)
    alpha = _linear22(*p["alpha"], h, False, variant)
    wd, bd = p["dir0"]
    if fold:
        wf, bf = p["feature"]
        with np.errstate(over="ignore", invalid="ignore"):
            w2 = np.concatenate([(wd[:, :arch.W].astype(np.float64) @ wf.astype(np.float64)).astype(np.float32), wd[:, arch.W:]], -1)
            b2 = (wd[:, :arch.W].astype(np.float64) @ bf.astype(np.float64) + bd.astype(np.float64)).astype(np.float32)
        hd = _linear22(w2, b2, np.concatenate([h, xd], -1), True, variant)
    else:
        feat = _linear22(*p["feature"], h, False, variant)
        hd = _linear22(wd, bd, np.concatenate([feat, xd], -1), True, variant)
    rgb = _linear22(*p["rgb"], hd, False, variant)
    return torch.from_numpy(np.concatenate([rgb, alpha], -1))


def oracle64(arch, flat, x):
    with torch.no_grad():
        return O.nerf_forward(arch, O.unflatten_params(arch, flat.double()), x.double())


def emulate22(arch, flat, x, fold=True, variant=None):
    """(E_emu, finite): max |emulated - oracle| / max |oracle| over the rows whose four outputs are finite (nan when there is none),
    and the [M, 4] mask of finite outputs."""
    got = emulate22_forward(arch, flat, x, fold, variant).double()
    want = oracle64(arch, flat.cpu(), x.cpu())
    finite = torch.isfinite(got)
    ok = finite.all(-1)
    e = float((got[ok] - want[ok]).abs().max() / want.abs().max()) if bool(ok.any()) else float("nan")
    return e, finite


def table_inputs():
    """(arch, flat, x) of the committed table: the view model and the embedded rows of the GPU test."""
    arch, flat = view_flat()
    return arch, flat, rows(*rays_z(B_RAYS, N_DEPTHS, SEED))


# E_emu(family, k), measured by emulate22 (folded stream) on table_inputs(); tests/test_range_host.py recomputes every entry.
# ("act", 15): over the rows the emulation leaves finite.
E_EMU = {
    ("act", 0): 1.1898e-07, ("act", 4): 3.5702e-07, ("act", -4): 2.9961e-07, ("act", 7): 6.4556e-06, ("act", -7): 5.0580e-06,
    ("act", 8): 1.3109e-05, ("act", -8): 1.2916e-05, ("act", 10): 1.0608e-04, ("act", -10): 1.1608e-04, ("act", 12): 3.4874e-04,
    ("act", -12): 2.1162e-04, ("act", 14): 3.4874e-04, ("act", -14): 2.1186e-04, ("act", 15): 3.4874e-04,
    ("alt", 0): 1.1898e-07, ("alt", 4): 2.2771e-07, ("alt", -4): 1.8164e-07, ("alt", 7): 3.6000e-06, ("alt", -7): 4.7662e-06,
    ("alt", 8): 1.3027e-05, ("alt", -8): 1.2191e-05, ("alt", 10): 1.5256e-04, ("alt", -10): 7.8626e-05, ("alt", 12): 2.0102e-04,
    ("alt", -12): 1.7094e-04, ("alt", 14): 2.0104e-04, ("alt", -14): 1.7094e-04,
}
TABLE_SHIFTS = (0,) + tuple(s * k for k in WINDOW + DEGRADED for s in (1, -1))
FWD_BAR = 1e-4                  # the project's forward bar at precision 22 (tests/test_gpu_pass_coverage.py TOL[22]["fwd"])


def degraded_bound(family, k):
    """E_emu(family, k) + the forward bar: the representation error the emulation models plus what it leaves out (fp32 accumulation
    order, the kernel's own sine).  An overflow case without finite emulated rows takes the family's largest degraded entry."""
    e = E_EMU.get((family, k))
    if e is None:
        e = max(E_EMU[(family, s * d)] for d in DEGRADED for s in (1, -1))
    return e + FWD_BAR
