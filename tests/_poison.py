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
