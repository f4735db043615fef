"""Poisoned buffers for the GPU tests (a helper module, not a conftest).

The product methods allocate their outputs with `torch.empty`, and the caching allocator hands a repeated call of the same shape
the block that holds the previous result: a pass a kernel skipped would then read as correct.  The callers below launch the same
C ABI entry points with the same arguments as `NeRF.query / forward / backward` and `HashNeRF.query`, but
  * every output is filled with SENTINEL first (a quiet NaN whose payload no kernel produces: a NaN a kernel computes from a NaN
    input is the canonical 0x7FC00000 or its negative), so `unwritten(out)` counts the elements nobody wrote;
  * every workspace (`acts`, `dz`) is filled with a byte pattern first.  A workspace is caller scratch of unspecified content: a
    result that differs between PATTERNS read scratch it never wrote.
"""
import ctypes as C

import torch

from nerf_meets_mlx_amd import _native as N

NAN_BYTES = 0xFF            # 0xFFFF... : NaN in every fp32, bf16 and fp16 view
BIG_BYTES = 0x7F            # 0x7F7F7F7F = 3.4e38 in fp32 (bf16 0x7F7F = 3.4e38, fp16 0x7F7F = NaN)
PATTERNS = (NAN_BYTES, BIG_BYTES)
SENTINEL = 0x7FE5A5A5


def poison_(t: torch.Tensor, pattern: int) -> torch.Tensor:
    """Fill the bytes of `t` (contiguous) with `pattern` in place."""
    t.view(torch.uint8).fill_(pattern)
    return t


def sentinel_(t: torch.Tensor) -> torch.Tensor:
    t.view(torch.int32).fill_(SENTINEL)
    return t


def unwritten(t: torch.Tensor) -> int:
    """Elements of a float32 tensor that still hold SENTINEL."""
    return int((t.contiguous().view(torch.int32) == SENTINEL).sum())


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bit-identical (NaN payloads included)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _out(shape, device):
    return sentinel_(torch.empty(*shape, dtype=torch.float32, device=device))


def _acts(m, M, pattern):
    """`m._begin_train_pass(M)` (the new generation that `backward()` checks), poisoned."""
    return poison_(m._begin_train_pass(M), pattern)


def query_into(m, rays, z, pattern, train=False, ref_quirks=True):
    """`NeRF.query` -> raw [B, n, 4] through `nerf_query_fused`."""
    B, n = z.shape
    raw = _out((B, n, 4), z.device)
    acts = _acts(m, B * n, pattern) if train else None
    N.check(N.lib().nerf_query_fused(C.byref(m.arch), N.ptr(m.packed()), N.ptr(rays), N.ptr(z), B, n, 0 if ref_quirks else 1,
                                     N.ptr(raw), N.ptr(acts), N.stream()))
    return raw


def forward_into(m, x, pattern, train=False):
    """`NeRF.forward` on embedded rows -> [M, out_dim] through `nerf_mlp_forward` / `nerf_mlp_forward_train`."""
    x = N.f32(x).reshape(-1, x.shape[-1])
    M = x.shape[0]
    out = _out((M, m.out_dim), x.device)
    if train:
        N.check(N.lib().nerf_mlp_forward_train(C.byref(m.arch), N.ptr(m.packed()), N.ptr(x), M, N.ptr(out),
                                               N.ptr(_acts(m, M, pattern)), N.stream()))
    else:
        N.check(N.lib().nerf_mlp_forward(C.byref(m.arch), N.ptr(m.packed()), N.ptr(x), M, N.ptr(out), N.stream()))
    return out


def backward_into(m, d_raw, pattern, need_input_grad=False):
    """`NeRF.backward` -> grads (m.grads, sentinel-filled first) [, d_x] through `nerf_mlp_backward` / `_inputs`."""
    d_raw = N.f32(d_raw)
    M = d_raw.numel() // m.out_dim
    assert M == m._acts_M, "backward_into() needs a matching train-mode forward first"
    dz = poison_(m._workspace("dz", N.lib().nerf_mlp_dz_bytes(C.byref(m.arch), M)), pattern)
    sentinel_(m.grads)
    if need_input_grad:
        d_x = _out((M, m.channel_input_pos), d_raw.device)
        N.check(N.lib().nerf_mlp_backward_inputs(C.byref(m.arch), N.ptr(m.packed()), N.ptr(m._ws["acts"]), N.ptr(d_raw), M,
                                                 N.ptr(dz), N.ptr(m.grads), N.ptr(d_x), N.stream()))
        return m.grads, d_x
    N.check(N.lib().nerf_mlp_backward(C.byref(m.arch), N.ptr(m.packed()), N.ptr(m._ws["acts"]), N.ptr(d_raw), M, N.ptr(dz),
                                      N.ptr(m.grads), N.stream()))
    return m.grads


def layer_into(m, kind, layer):
    """`debug_layer` with a sentinel-filled output: one layer of the last training stores as row-major [M, width]."""
    k = {"acts": 0, "dz": 1}[kind]
    w = N.lib().nerf_mlp_debug_width(C.byref(m.arch), k, layer)
    assert w > 0, (kind, layer)
    out = _out((m._acts_M, w), m.device)
    N.check(N.lib().nerf_mlp_debug_read(C.byref(m.arch), N.ptr(m._ws[kind]), k, layer, m._acts_M, N.ptr(out), N.stream()))
    return out


def ngp_query_into(f, rays, z, pattern, train=False):
    """`HashNeRF.query` (fused) -> raw [B, n, 4] through `nerf_ngp_query_fused_h`."""
    B, n = z.shape
    e, m = f.enc, f.mlp
    rays, z = N.f32(rays), N.f32(z)
    raw = _out((B, n, 4), z.device)
    acts = None
    if train:
        acts = _acts(m, B * n, pattern)
        f._pts, f._rz = None, (rays, z)
    N.check(N.lib().nerf_ngp_query_fused_h(C.byref(m.arch), N.ptr(m.packed()), N.ptr(rays), N.ptr(z), B, n, N.ptr(e.tables),
                                           N.ptr(f.table.shadow()), e.n_levels, e.log2_hashmap_size, e.n_features_per_level,
                                           e._res_c, 3, f.pos_scale, f.pos_offset, N.ptr(raw), N.ptr(acts), N.stream()))
    return raw


# ---- the volume renderer (csrc/sampling.hip, csrc/composite.hip): same C ABI calls as sampling / rendering.render / ops.metric,
# every requested output sentinel-filled first; an output not named in `want` is passed as NULL.  Loss words are accumulated
# into by the kernels (the caller zeroes them), so they start at 0, not at the sentinel.
def sample_coarse_into(rays, n, lindisp=False, perturb=0.0, t_rand=None):
    B = rays.shape[0]
    z = _out((B, n), rays.device)
    N.check(N.lib().nerf_sample_coarse(N.ptr(rays), B, n, int(lindisp), float(perturb), N.ptr(t_rand), N.ptr(z), N.stream()))
    return z


def add_noise_z_into(z, t_rand, strength):
    B, n = z.shape
    out = _out((B, n), z.device)
    N.check(N.lib().nerf_add_noise_z(N.ptr(z), N.ptr(t_rand), B, n, float(strength), N.ptr(out), N.stream()))
    return out


def importance_into(z, w, u, eps=1e-5, want=("z_new", "z_merged", "cdf", "inds")):
    """dict of the requested outputs of `nerf_importance_sample` (inds: int64, sentinel words in both halves)."""
    (B, n), Ns = z.shape, u.shape[1]
    o = {"z_new": _out((B, Ns), z.device), "z_merged": _out((B, n + Ns), z.device), "cdf": _out((B, n + 1), z.device),
         "inds": sentinel_(torch.empty(B, Ns, dtype=torch.int64, device=z.device))}
    o = {k: v for k, v in o.items() if k in want}
    N.check(N.lib().nerf_importance_sample(N.ptr(z), N.ptr(w), N.ptr(u), B, n, Ns, float(eps), N.ptr(o.get("z_new")),
                                           N.ptr(o.get("z_merged")), N.ptr(o.get("cdf")), N.ptr(o.get("inds")), N.stream()))
    return o


FWD_OUTPUTS = ("rgb", "disp", "acc", "weights", "depth")


def composite_forward_into(raw, z, rays, white=False, noise=None, raw_noise_std=0.0, want=FWD_OUTPUTS):
    B, n = z.shape
    o = {"rgb": _out((B, 3), z.device), "disp": _out((B,), z.device), "acc": _out((B,), z.device),
         "weights": _out((B, n), z.device), "depth": _out((B,), z.device)}
    o = {k: v for k, v in o.items() if k in want}
    N.check(N.lib().nerf_composite_forward(N.ptr(raw), N.ptr(z), N.ptr(rays), B, n, float(raw_noise_std), N.ptr(noise),
                                           int(white), N.ptr(o["rgb"]), N.ptr(o.get("disp")), N.ptr(o.get("acc")),
                                           N.ptr(o.get("weights")), N.ptr(o.get("depth")), N.stream()))
    return o


def composite_backward_into(raw, z, rays, d_rgb, d_acc=None, d_depth=None, white=False, noise=None, raw_noise_std=0.0):
    B, n = z.shape
    d_raw = _out((B, n, 4), z.device)
    N.check(N.lib().nerf_composite_backward(N.ptr(raw), N.ptr(z), N.ptr(rays), B, n, float(raw_noise_std), N.ptr(noise),
                                            int(white), N.ptr(d_rgb), N.ptr(d_acc), N.ptr(d_depth), N.ptr(d_raw), N.stream()))
    return d_raw


def composite_mse_backward_into(raw, z, rays, target, white=False, grad_scale=1.0, want_rgb=True, want_loss=True):
    """(loss [1] or None, rgb [B, 3] or None, d_raw [B, n, 4]) of `nerf_composite_mse_backward`."""
    B, n = z.shape
    d_raw = _out((B, n, 4), z.device)
    rgb = _out((B, 3), z.device) if want_rgb else None
    loss = torch.zeros(1, dtype=torch.float32, device=z.device) if want_loss else None
    N.check(N.lib().nerf_composite_mse_backward(N.ptr(raw), N.ptr(z), N.ptr(rays), B, n, int(white), N.ptr(target),
                                                float(grad_scale), N.ptr(loss), N.ptr(rgb), N.ptr(d_raw), N.stream()))
    return loss, rgb, d_raw


def mse_loss_grad_into(p, t, grad_scale=1.0, want_grad=True, want_loss=True):
    """(loss [1] or None, d_pred or None) of `nerf_mse_loss_grad`."""
    grad = _out(tuple(p.shape), p.device) if want_grad else None
    loss = torch.zeros(1, dtype=torch.float32, device=p.device) if want_loss else None
    N.check(N.lib().nerf_mse_loss_grad(N.ptr(p), N.ptr(t), p.numel(), float(grad_scale), N.ptr(loss), N.ptr(grad), N.stream()))
    return loss, grad
