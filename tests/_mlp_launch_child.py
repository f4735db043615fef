"""Child process of tests/test_gpu_mlp_launch.py: every MLP kernel instantiation of the library once, in a fresh process (the
once-per-kernel opt-ins to dynamic LDS above 64 KiB start unset).  argv[1] = "infer-first" | "train-first": which half runs
first.  Prints one JSON line: {"error": nerf_last_error(), "digests": {case: sha256}}; the digests do not depend on the order."""
import ctypes as C
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nerf_meets_mlx_amd import _native as N  # noqa: E402
from oracle import nerf_oracle as O  # noqa: E402

DEV, M, B, NS = "cuda", 65, 64, 3
# the models of tools/ab_libs.py --models
SHAPES = {"view": (8, 256, 63, 27, 4, 1, 4), "image": (8, 256, 40, 0, 4, 0, 3), "small": (2, 64, 32, 16, -1, 1, 4)}
MODELS = [(s, p) for s in SHAPES for p in (16, 32, 22) if (s, p) != ("small", 32)]
lib, digests = N.lib(), {}


def sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def zeros(n, dt=torch.uint8):
    return torch.zeros(n, dtype=dt, device=DEV)


class Options:
    """nerf_set_option for the duration of a with block."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.before = {k: lib.nerf_get_option(k.encode()) for k in self.kv}
        for k, v in self.kv.items():
            N.check(lib.nerf_set_option(k.encode(), v))

    def __exit__(self, *exc):
        for k, v in self.before.items():
            N.check(lib.nerf_set_option(k.encode(), v))


class Net:
    def __init__(self, shape, prec):
        self.shape, self.prec, self.name = shape, prec, f"{shape}{prec}"
        g = torch.Generator().manual_seed(1000 * prec + len(shape))
        self.arch = N.MlpArch(*SHAPES[shape], prec)
        self.a = a = C.byref(self.arch)
        self.params = (torch.randn(lib.nerf_mlp_param_count(a), generator=g) * 0.05).to(DEV)
        self.packed = zeros(lib.nerf_mlp_packed_bytes(a))
        N.check(lib.nerf_mlp_pack(a, N.ptr(self.params), N.ptr(self.packed), N.stream()))
        self.cin, self.cout = self.arch.in_pos + self.arch.in_dir, self.arch.out_ch
        self.x = (torch.randn(M, self.cin, generator=g) * 0.5).to(DEV)
        self.d_out = torch.randn(M, self.cout, generator=g).to(DEV)
        o = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=-1) * 4.0
        self.rays = O.pack_rays(o, -o / 4.0 + 0.25 * torch.randn(B, 3, generator=g), 2.0, 6.0).to(DEV)
        self.z = (torch.sort(torch.rand(B, NS, generator=g), -1).values * 4 + 2).to(DEV)
        if shape == "small":
            self.tables = (torch.randn(16 * (1 << 14) * 2, generator=g) * 0.1).to(DEV)
            self.tables_h = self.tables.to(torch.float16)
            self.reso = (C.c_int * 16)(*[int(16 * (2048 / 16) ** (l / 15)) for l in range(16)])
            self.lw = (C.c_float * 16)(*[1.0] * 12 + [0.75, 0.5, 0.25, 0.0])
        digests[f"{self.name} packed"] = sha(self.packed)

    def rows(self, tag, train):
        """nerf_mlp_forward (train False) or nerf_mlp_forward_train + backward + the test hook's read of both stores."""
        a, out = self.a, zeros(M * self.cout, torch.float32)
        if not train:
            N.check(lib.nerf_mlp_forward(a, N.ptr(self.packed), N.ptr(self.x), M, N.ptr(out), N.stream()))
            digests[f"{self.name} rows infer {tag}"] = sha(out)
            return
        acts, dz = zeros(lib.nerf_mlp_acts_bytes(a, M)), zeros(lib.nerf_mlp_dz_bytes(a, M))
        grads, d_x = zeros(self.params.numel(), torch.float32), zeros(M * self.arch.in_pos, torch.float32)
        N.check(lib.nerf_mlp_forward_train(a, N.ptr(self.packed), N.ptr(self.x), M, N.ptr(out), N.ptr(acts), N.stream()))
        if self.shape == "small":
            N.check(lib.nerf_mlp_backward_inputs(a, N.ptr(self.packed), N.ptr(acts), N.ptr(self.d_out), M, N.ptr(dz), N.ptr(grads),
                                                 N.ptr(d_x), N.stream()))
        else:
            N.check(lib.nerf_mlp_backward(a, N.ptr(self.packed), N.ptr(acts), N.ptr(self.d_out), M, N.ptr(dz), N.ptr(grads), N.stream()))
        read = []
        for kind, store in ((0, acts), (1, dz)):
            width = lib.nerf_mlp_debug_width(a, kind, 1)
            assert width > 0, (self.name, kind)
            read.append(zeros(M * width, torch.float32))
            N.check(lib.nerf_mlp_debug_read(a, N.ptr(store), kind, 1, M, N.ptr(read[-1]), N.stream()))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(grads).all()) and float(grads.abs().max()) > 0, (self.name, tag)
        partial = 2048 * (4096 + 64) * 4 if self.prec == 32 else 512 * (64 * 1024 + 256) * 4   # split-K partial slots behind the dZ blocks
        for what, t in (("out", out), ("acts", acts), ("dz", dz[:dz.numel() - partial]), ("grads", grads), ("d_x", d_x),
                        ("read acts", read[0]), ("read dz", read[1])):
            digests[f"{self.name} rows train {tag} {what}"] = sha(t)

    def fused(self, tag, train, weighted=False, half=False):
        """nerf_query_fused (view) or nerf_ngp_query_fused / _h / _lw (2 x 64) at B x NS samples."""
        a, raw = self.a, zeros(B * NS * 4, torch.float32)
        acts = zeros(lib.nerf_mlp_acts_bytes(a, B * NS)) if train else None
        if self.shape == "view":
            N.check(lib.nerf_query_fused(a, N.ptr(self.packed), N.ptr(self.rays), N.ptr(self.z), B, NS, 0, N.ptr(raw), N.ptr(acts), N.stream()))
        else:
            head = (a, N.ptr(self.packed), N.ptr(self.rays), N.ptr(self.z), B, NS, N.ptr(self.tables))
            tail = (3, 1.0 / 12.0, 0.5, N.ptr(raw), N.ptr(acts), N.stream())
            if weighted:
                N.check(lib.nerf_ngp_query_fused_lw(*head, N.ptr(self.tables_h) if half else None, 16, 14, 2, self.reso, self.lw, *tail))
            elif half:
                N.check(lib.nerf_ngp_query_fused_h(*head, N.ptr(self.tables_h), 16, 14, 2, self.reso, *tail))
            else:
                N.check(lib.nerf_ngp_query_fused(*head, 16, 14, 2, self.reso, *tail))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(raw).all()), (self.name, tag)
        key = f"{self.name} fused {'train' if train else 'infer'} {tag}{' lw' if weighted else ''}{' half' if half else ''}"
        digests[key] = sha(raw)
        if train:
            digests[key + " acts"] = sha(acts)


def half_of(nets, train):
    """Every launch of one half (inference: no stores kept; training: forward with stores, backward, store reads)."""
    for net in nets:
        net.rows("default", train)
        if net.shape == "image":
            continue
        net.fused("default", train)
        if net.shape == "small":
            net.fused("default", train, weighted=True)
            if net.prec == 16:                   # the fp16 shadow tables are a precision-16 option
                net.fused("default", train, half=True)
                net.fused("default", train, weighted=True, half=True)
        if net.name == "view16":
            for v in (1, 2, 3) if train else (1, 2, 3, 4, 5):          # 4 and 5 are inference forms
                with Options(mlp_variant=v):
                    net.rows(f"mlp_variant={v}", train)
                    net.fused(f"mlp_variant={v}", train)
            if train:
                with Options(ring_split=2):
                    net.rows("ring_split=2", train)
                    net.fused("ring_split=2", train)
                with Options(dw16_variant=0):
                    net.rows("dw16_variant=0", train)
        if net.name == "small16" and train:
            with Options(dw16_variant=0):
                net.rows("dw16_variant=0", train)
        if net.name == "view22":
            if train:
                with Options(dw22_variant=0):
                    net.rows("dw22_variant=0", train)
            else:
                for t in (2, 3):
                    with Options(f22_tiles=t):
                        net.fused(f"f22_tiles={t}", train)


order = {"infer-first": (False, True), "train-first": (True, False)}[sys.argv[1]]
nets = [Net(s, p) for s, p in MODELS]
for train in order:
    half_of(nets, train)
torch.cuda.synchronize()
print(json.dumps({"error": lib.nerf_last_error().decode(errors="replace"), "digests": digests}))
